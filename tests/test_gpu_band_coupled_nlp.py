"""Coupled quadratic constraints on the device-resident nonlinear model of the banded back-end (fpsq_band_nlp_create_coupled,
DeviceBandCoupledQuadNLP).  The yardstick is the CPU restatement tests/coupled_quad_ref.py (tests/sepquad_ref.py on
nlpmodels.CoupledQuadConModel: exact KKT solves at J(x), the gradient in the -ys form, the mirror's hprod_), at the bars
tests/test_gpu_band_nlp.py holds this back-end to: max|a - b| / max|b| < 1e-9 per vector, |fx - fx_ref| <= 1e-9 |fx_ref|.
Dropping the terms moves the reference gx and Hv by more than 1e-3 on every case (tests/test_band_coupled_nlp_cpu.py), so the
bar tells the two models apart.  The cases: tests/coupled_cases.py.

Second trips of the grid-stride loops: the case `stride` takes k_bcn_vals (both launches), k_bn_prologue<LG, true>,
k_bn_epilogue<LG, true>, k_bcn_finish, k_bcn_hcv, k_bn_epilogue_h1<LG, true>, k_bcn_finish_h1, k_bn_hgv<LG, true> and
k_bn_cons<LG, true> through theirs; k_bcn_assemble's takes nnz(S) > 1048576 (with one term per row N > 524288) and is reached by
the case assemble-stride of tests/test_gpu_coupled_lane_groups.py, which also runs these kernels at every lane-group width."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
import coupled_cases as cc  # noqa: E402
from coupled_quad_ref import CoupledQuadRef  # noqa: E402
from fps_amd import _lib, nlpmodels, problems  # noqa: E402
from fps_amd.device_qp import (DeviceBandCoupledQuadNLP, DeviceBandEqQP, DeviceBandSepQuadNLP,  # noqa: E402
                               DeviceBorderedBandEqQP)
from fps_amd.qdsolver import FpsqError  # noqa: E402
from lane_group_cases import lane_group, tiles  # noqa: E402

pytestmark = pytest.mark.gpu

SE, SIGMA = cc.SE, cc.SIGMA
ERR_ARG, ERR_STATE = -1, -3


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _objgrad(dev, x, xk, on=None):
    """one evaluation with every output; `on`: a torch device to run it on device tensors, None: numpy arrays"""
    qp = dev.qp
    if on is None:
        gx, ys, gs = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
        fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xk)
        return fx, rc, gx, ys, gs
    import torch

    # (the cases' arrays are read-only: copies)
    t = lambda a: None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).to(on)  # noqa: E731
    gx, ys, gs = (torch.empty(k, dtype=torch.float64, device=on) for k in (qp.n, qp.m, qp.n))
    fx, rc = dev.objgrad(t(x), gx=gx, ys=ys, gs=gs, xk=t(xk))
    return fx, rc, gx.cpu().numpy(), ys.cpu().numpy(), gs.cpu().numpy()


def _check_against_the_restatement(name, data, delta, pairs, want_info):
    """objgrad, hprod Val(2) and Val(1), cons against the yardstick for the given (rho, eta) pairs; then jac_mul on J(x)"""
    qp = data.qp
    x, xk = qp.x, qp.xhat
    dev = DeviceBandCoupledQuadNLP(data, sigma=SIGMA, rho=0.0, delta=delta, eta=0.0)
    info = dev.info()
    for k, v in want_info.items():
        assert info[k] == v, (k, info)
    assert info["border_rows"] == 0 and info["border_cols"] == 0
    ref = CoupledQuadRef(data, SIGMA, 0.0, delta, 0.0, xk, keep_factors=True)   # (ys, gs, c depend on sigma and delta alone)
    v = np.random.default_rng(0).standard_normal(qp.n)
    c = np.empty(qp.m)
    assert dev.cons(x, c) == 0
    nobj = 0
    for rho, eta in pairs:
        dev.rho, dev.eta = rho, eta
        ref.pen.rho, ref.pen.eta = rho, eta
        fx, rc, gx, ys, gs = _objgrad(dev, x, xk)
        nobj += 1
        e = ref.objgrad(x)
        errs = {"gx": _rel(gx, e["gx"]), "ys": _rel(ys, e["ys"]), "gs": _rel(gs, e["gs"]), "c": _rel(c, e["c"]),
                "fx": abs(fx - e["fx"]) / abs(e["fx"])}
        Hv2, Hv1 = np.empty(qp.n), np.empty(qp.n)
        assert dev.hprod(v, Hv2, 2) == 0 and dev.hprod(v, Hv1, 1) == 0
        errs["Hv2"] = _rel(Hv2, ref.hprod(x, v, 2))
        errs["Hv1"] = _rel(Hv1, ref.hprod(x, v, 1))
        errs["Hv1-Hv2"] = _rel(Hv1, Hv2)
        print(f"\n{name} delta={delta:.1e} rho={rho} eta={eta}: " + " ".join(f"{k}={v_:.2e}" for k, v_ in errs.items()))
        assert rc == 0
        for k in ("gx", "ys", "gs", "c", "Hv2", "Hv1"):
            assert errs[k] < 1e-9, (k, errs[k])
        assert abs(fx - e["fx"]) <= 1e-9 * abs(e["fx"])
        assert errs["Hv1-Hv2"] > 1e-6
    assert dev.info()["factorizations"] == nobj   # one per objgrad, none for hprod / cons
    # the handle's values are J(x) now, terms included: fpsq_band_jac_mul multiplies with it
    J = nlpmodels.CoupledQuadConModel(data)._J(x)
    u, y, z = np.random.default_rng(2).standard_normal(qp.m), np.empty(qp.m), np.empty(qp.n)
    assert dev.jac_mul(0, 1.0, v, 0.0, y) == 0 and dev.jac_mul(1, 1.0, u, 0.0, z) == 0
    assert _rel(y, J @ v) < 1e-13 and _rel(z, J.T @ u) < 1e-13
    dev.close()


@pytest.mark.parametrize("delta", [0.0, SE], ids=["delta0", "deltaSE"])
@pytest.mark.parametrize("case", list(cc.CASES))
def test_objgrad_hprod_and_cons_match_the_exact_restatement(case, delta):
    """Val(1) at delta = sqrt(eps) is the same quantity as the mirror's (tau = delta); at delta = 0 the mirror solves with
    tau = 1e-14 and the device with the cached factor (tau = 0): they differ by O(1e-14 |M^-1|), far inside the bar."""
    data = cc.data(case)
    assert (data.qp.m % 128 == 0) == (case == "m-multiple-of-128")
    if case == "hub":
        rows, snz, longest = cc.s_pattern(data)
        assert lane_group(snz, data.qp.n) == 8 and longest > 16 * 8
    if case == "sparse-terms":
        assert cc.s_pattern(data)[0] < data.qp.n // 4 and data.nterms < data.qp.m
    _check_against_the_restatement(case, data, delta, ((0.0, 0.0), (1.0, 0.5)), cc.CASES[case][1])


def test_second_trip_of_the_grid_stride_loops():
    """the case `stride` (coupled_cases.py): more row tiles than kBqMaxGrid on the rows of A, of A' and of S, more entries than
    4096 workgroups of k_bcn_vals take in one trip; one delta, one (rho, eta)"""
    data = cc.data("stride")
    qp = data.qp
    snz = cc.s_pattern(data)[1]
    mpad = 128 * ((qp.m + 127) // 128)
    assert tiles(mpad, lane_group(qp.nnz, qp.m)) > 2048 and tiles(qp.n, lane_group(qp.nnz, qp.n)) > 2048
    assert tiles(qp.n, lane_group(snz, qp.n)) > 2048 and qp.nnz > 4096 * 256
    _check_against_the_restatement("stride", data, SE, ((1.0, 0.5),), {})


def test_without_terms_the_model_is_the_separable_one_bit_for_bit():
    """nterms = 0: fpsq_band_nlp_create_coupled runs fpsq_band_nlp_create's launches"""
    sep = cc.without_terms(cc.data("small"))
    qp = sep.qp
    none = problems.CoupledQuadNLP(qp, sep.hvals, sep.b, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                                   np.zeros(0))
    x, xk = qp.x, qp.xhat
    v = np.random.default_rng(0).standard_normal(qp.n)
    outs = []
    for cls, d in ((DeviceBandSepQuadNLP, sep), (DeviceBandCoupledQuadNLP, none)):
        dev = cls(d, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
        got = list(_objgrad(dev, x, xk))
        assert got[1] == 0
        for ha in (2, 1):
            H = np.empty(qp.n)
            assert dev.hprod(v, H, ha) == 0
            got.append(H)
        c = np.empty(qp.m)
        assert dev.cons(x, c) == 0
        got.append(c)
        assert dev.info()["factorizations"] == 1
        outs.append(got)
        dev.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", ["small", "row-shuffled"])
def test_linear_limit_agrees_with_the_linear_model(case):
    """h_vals = 0 and every w = 0 WITH THE TERMS PRESENT (the coupled launches run on lists of zeros): the model is the eq-QP,
    objgrad / hprod agree with DeviceBandEqQP within 1e-12 relative, Val(1) equals Val(2) within that."""
    full = cc.data(case)
    qp = full.qp
    data = dataclasses.replace(full, hvals=np.zeros_like(qp.vals), b=qp.b.copy(), t_w=np.zeros_like(full.t_w))
    assert data.nterms > 0
    x, xk = qp.x, qp.xhat
    v = np.random.default_rng(0).standard_normal(qp.n)
    for delta in (0.0, SE):
        lin = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
        dev = DeviceBandCoupledQuadNLP(data, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
        a, b = _objgrad(lin, x, xk), _objgrad(dev, x, xk)
        assert a[1] == 0 and b[1] == 0
        assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
        for p, q in zip(a[2:], b[2:]):
            assert _rel(q, p) < 1e-12
        Hl, H2, H1 = np.empty(qp.n), np.empty(qp.n), np.empty(qp.n)
        assert lin.hprod(v, Hl, 2) == 0 and dev.hprod(v, H2, 2) == 0 and dev.hprod(v, H1, 1) == 0
        assert _rel(H2, Hl) < 1e-12 and _rel(H1, H2) < 1e-12
        assert dev.info()["factorizations"] == 1
        lin.close()
        dev.close()


def test_repeatability_placement_and_no_state_between_evaluations():
    import torch

    data = cc.data("small")
    qp = data.qp
    x1, x2, xk = qp.x, qp.point(2), qp.xhat
    on = torch.device("cuda", 0)
    v = np.random.default_rng(1).standard_normal(qp.n)

    def hprods(dev, device_args):
        out = []
        for ha in (2, 1):
            if device_args:
                H = torch.empty(qp.n, dtype=torch.float64, device=on)
                assert dev.hprod(torch.from_numpy(v).to(on), H, ha) == 0
                out.append(H.cpu().numpy())
            else:
                H = np.empty(qp.n)
                assert dev.hprod(v, H, ha) == 0
                out.append(H)
        return out

    dev = DeviceBandCoupledQuadNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    host = _objgrad(dev, x1, xk)
    hh = hprods(dev, False)
    again = _objgrad(dev, x1, xk)
    devt = _objgrad(dev, x1, xk, on=on)
    hd = hprods(dev, True)
    assert host[1] == 0
    for a, b, c in zip(host, again, devt):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    for a, b in zip(hh, hd):
        assert np.array_equal(a, b)
    ch, cd = np.empty(qp.m), torch.empty(qp.m, dtype=torch.float64, device=on)
    assert dev.cons(x1, ch) == 0 and dev.cons(torch.from_numpy(x1.copy()).to(on), cd) == 0
    assert np.array_equal(ch, cd.cpu().numpy())
    # a second x: another J, other Wo values, and nothing of the first evaluation is left -- a fresh handle gives the same bits
    second = _objgrad(dev, x2, xk)
    h2 = hprods(dev, False)
    fresh_dev = DeviceBandCoupledQuadNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    fresh = _objgrad(fresh_dev, x2, xk)
    hf = hprods(fresh_dev, False)
    assert second[1] == 0 and fresh[1] == 0
    assert not np.array_equal(second[2], host[2])
    for a, b in zip(second, fresh):
        assert np.array_equal(a, b)
    for a, b in zip(h2, hf):
        assert np.array_equal(a, b)
    assert dev.info()["factorizations"] == 4 and fresh_dev.info()["factorizations"] == 1
    dev.close()
    fresh_dev.close()


def test_state_rules():
    lib = _lib.load()
    data = cc.data("small")
    qp = data.qp
    x, xk = qp.x, qp.xhat
    v, Hv = np.random.default_rng(1).standard_normal(qp.n), np.empty(qp.n)
    dev = DeviceBandCoupledQuadNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.0)
    h, q = dev._h, dev._q

    def hprod_rc(ha=2):
        return lib.fpsq_band_nlp_hprod(h, q, v.ctypes.data, SIGMA, 1.0, 0.0, ha, Hv.ctypes.data)

    assert hprod_rc() == ERR_STATE and b"objgrad" in lib.fpsq_band_last_error(h)
    assert hprod_rc(1) == ERR_STATE
    with pytest.raises(FpsqError):
        dev.hprod(v, Hv)
    first = _objgrad(dev, x, xk)
    assert first[1] == 0 and hprod_rc() == 0 and hprod_rc(1) == 0
    assert hprod_rc(3) == ERR_ARG
    # someone else factorises the handle: the model's point is gone until its next objgrad, which returns what it returned
    assert lib.fpsq_band_factorize(h, qp.vals.ctypes.data, SE, None) == 0
    assert hprod_rc() == ERR_STATE and b"factorised again" in lib.fpsq_band_last_error(h)
    assert hprod_rc(1) == ERR_STATE
    back = _objgrad(dev, x, xk)
    for a, b in zip(first, back):
        assert np.array_equal(a, b)
    assert hprod_rc() == 0 and hprod_rc(1) == 0
    assert dev.info()["factorizations"] == 2
    dev.close()


def _create_rc(lib, handle, prob, hvals, t_row, t_j, t_k, t_w):
    out = C.c_void_p()
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    t_row, t_j, t_k, t_w = i32(t_row), i32(t_j), i32(t_k), np.ascontiguousarray(t_w, dtype=np.float64)
    rc = lib.fpsq_band_nlp_create_coupled(handle, prob.qdiag.ctypes.data, prob.d.ctypes.data, prob.b.ctypes.data,
                                          prob.vals.ctypes.data, hvals.ctypes.data, t_w.size, t_row.ctypes.data, t_j.ctypes.data,
                                          t_k.ctypes.data, t_w.ctypes.data, C.byref(out))
    msg = lib.fpsq_band_last_error(handle)
    if rc == 0:
        assert lib.fpsq_band_nlp_destroy(out) == 0
    return rc, msg


def test_create_time_refusals():
    lib = _lib.load()
    data = cc.data("row-shuffled")       # (a reordered handle: the pattern check goes through the row permutation)
    qp = data.qp
    dev = DeviceBandCoupledQuadNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.0)
    assert dev.info()["reordered"] == 1
    h = dev._h
    row0 = qp.colind[qp.rowptr[0]:qp.rowptr[1]]
    off = int(np.setdiff1d(np.arange(qp.n), row0)[0])       # a column row 0 does not hold
    j0, k0, k1 = int(row0[0]), int(row0[1]), int(row0[2])
    good = ([0, 0], [j0, j0], [k0, k1], [0.1, 0.2])
    assert _create_rc(lib, h, qp, data.hvals, *good)[0] == 0
    bad = {
        "row below range": (([-1], [j0], [k0], [0.1]), b"out of range"),
        "row above range": (([qp.m], [j0], [k0], [0.1]), b"out of range"),
        "column below range": (([0], [-1], [k0], [0.1]), b"out of range"),
        "column above range": (([0], [j0], [qp.n], [0.1]), b"out of range"),
        "j = k": (([0], [j0], [j0], [0.1]), b"j = k"),
        "pair twice": (([0, 1, 0], [j0, int(qp.colind[qp.rowptr[1]]), j0], [k0, int(qp.colind[qp.rowptr[1] + 1]), k0],
                        [0.1, 0.1, 0.2]), b"listed twice"),
        "pair twice, swapped": (([0, 0], [j0, k0], [k0, j0], [0.1, 0.2]), b"listed twice"),
        "j off the pattern": (([0], [off], [k0], [0.1]), b"not an entry"),
        "k off the pattern": (([0], [j0], [off], [0.1]), b"not an entry"),
    }
    for what, (terms, needle) in bad.items():
        rc, msg = _create_rc(lib, h, qp, data.hvals, *terms)
        assert rc == ERR_ARG and b"band_nlp_create_coupled" in msg and needle in msg, (what, rc, msg)
    # the model made before the refusals still evaluates
    assert _objgrad(dev, qp.x, qp.xhat)[1] == 0
    dev.close()

    # handles the model does not take: border rows, long columns, COO-created -- fpsq_band_nlp_create's messages
    one = ([0], [0], [1], [0.0])
    big = problems.pde_control_like(n=12000, m=1280, per_row=16, window=512, seed=9)
    rows = DeviceBorderedBandEqQP(problems.with_border_rows(big, 2), border=16, cols=0)
    assert rows.info()["border_rows"] > 0
    rc, msg = _create_rc(lib, rows._h, rows.qp, np.zeros_like(rows.qp.vals), *one)
    assert rc == ERR_STATE and b"band_nlp_create" in msg and b"border rows" in msg
    rows.close()
    cols = DeviceBorderedBandEqQP(problems.with_long_columns(big, 2), border=0, cols=16)
    assert cols.info()["border_cols"] > 0
    rc, msg = _create_rc(lib, cols._h, cols.qp, np.zeros_like(cols.qp.vals), *one)
    assert rc == ERR_STATE and b"band_nlp_create" in msg and b"long columns" in msg
    cols.close()
    sq = cc.small_qp()
    coo = C.c_void_p()
    r = np.repeat(np.arange(sq.m, dtype=np.int64), np.diff(sq.rowptr))
    cidx = sq.colind.astype(np.int64)
    assert lib.fpsq_band_create_coo(C.byref(coo), sq.n, sq.m, sq.nnz, r.ctypes.data, cidx.ctypes.data, 0, 0) == 0
    rc, msg = _create_rc(lib, coo, sq, np.zeros_like(sq.vals), *one)
    assert rc == ERR_STATE and b"band_nlp_create" in msg and b"fpsq_band_create_coo" in msg
    assert lib.fpsq_band_destroy(coo) == 0


@pytest.mark.parametrize("sub", ["lbfgs", "trunk"])
@pytest.mark.parametrize("case", ["bilinear", "small"])
def test_fps_solve_device_end_to_end(case, sub):
    """tests/test_gpu_band_nlp.py's end-to-end test on the coupled model: from x0 = xhat + 0.1 (x - xhat), the returned point
    checked INDEPENDENTLY with the host model and the solver's own score rule: primal |c(x*)|inf / max(|x*|, 1), dual
    |grad f + J'lambda|inf / max(|lambda|, 1), both <= 10 tol, tol = max(atol, rtol max(p0, d0)), atol = rtol = sqrt(eps)."""
    import torch

    from fps_amd.fps_solve import fps_solve_device

    data = cc.data(case)
    qp = data.qp
    nlp = nlpmodels.CoupledQuadConModel(data)
    x0 = qp.xhat + 0.1 * (qp.x - qp.xhat)
    dev = DeviceBandCoupledQuadNLP(data)
    st = fps_solve_device(dev, torch.from_numpy(x0.copy()).to(torch.device("cuda", 0)), max_iter=30, subproblem_solver=sub)
    xs, lam = st.solution.cpu().numpy(), st.multipliers.cpu().numpy()
    p0 = np.abs(nlp.cons(x0)).max() / max(np.linalg.norm(x0), 1.0)
    d0 = np.abs(nlp.grad(x0)).max()
    tol = max(SE, SE * max(p0, d0))
    primal = np.abs(nlp.cons(xs)).max() / max(np.linalg.norm(xs), 1.0)
    dual = np.abs(nlp.grad(xs) + nlp.jtprod(xs, lam)).max() / max(np.linalg.norm(lam), 1.0)
    info = dev.info()
    print(f"\nfps_solve_device {case}/{sub}: {st.status} in {st.iter} outer iterations, primal {primal:.2e} dual {dual:.2e} "
          f"tol {tol:.2e}, {st.solver_specific}, factorizations {info['factorizations']}")
    assert st.status == "first_order"
    assert primal <= 10 * tol and dual <= 10 * tol
    assert info["factorizations"] == st.solver_specific["objgrad_calls"]
    dev.close()
