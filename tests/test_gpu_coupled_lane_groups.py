"""The coupled quadratic model (fpsq_band_nlp_create_coupled, DeviceBandCoupledQuadNLP) at every lane-group width on the rows
of A, of A' and of S, and k_bcn_assemble through its second grid-stride trip: each case of tests/coupled_lane_cases.py through
cons, one objgrad with every output, hprod Val(2) and Val(1), then jac_mul with both `trans` values on the handle's J(x) -- what
`_check_against_the_restatement` of tests/test_gpu_band_coupled_nlp.py does on the cases of tests/coupled_cases.py, which reach
lgA 2, 4, 16, 32, lgT 1, 2, 32 and lgR 1, 8 only.

The yardstick is tests/coupled_quad_ref.py with kept factors (exact sparse KKT solves at J(x) in fp64, no device code),
computed once per case and delta (coupled_lane_cases.expected); the bars are the ones of that suite and of
tests/test_gpu_lane_groups.py: max|a - b| / max|b| < 1e-9 for gx, ys, gs, c, Hv2, Hv1, |fx - ref| <= 1e-9 |ref|, jac_mul 1e-13,
and Val(1) differs from Val(2) by more than 1e-6.  info(): one factorisation per objgrad, no regularised pivot, the band as
pinned.  On assemble-stride the objgrad is run with host and with device arguments and must give the same bits.  Each test
prints its figures (COUPLED-LANES lines, pytest -s).

MEASURED on the MI355X, worst relative error per quantity over every case, delta and (rho, eta) (the case it occurs on):
  gx 6.3e-14 (ragged-r2)  ys 5.0e-14 (ragged-shuffled-r2)  gs 6.6e-14  c 1.3e-14  Hv2 3.5e-14  Hv1 3.5e-14 (assemble-stride)
  fx 6.0e-16 (both-64-shuffled-r16)  jac_mul J 1.2e-15 (ragged-shuffled-r2)  J' 8.5e-16 (both-64-r16)
  the smallest |Hv1 - Hv2| / |Hv2|: 8.2e-3 (assemble-stride)
  per case, the worst of its figures: thin-r2 5.9e-15, lg2-r4 2.5e-15, lg4-2-r1 4.0e-15, lg4-2-r2 5.0e-15, lg8-4-r3 1.1e-14,
  lg16-2-r8 6.5e-15, lgT-8-r2 1.0e-14, lgT-16-r4 2.5e-14, m-near-n-r1 2.3e-14, both-64-r16 3.5e-14, wide-rows-r1 3.5e-14,
  ragged-r2 6.4e-14, both-64-shuffled-r16 4.4e-14, ragged-shuffled-r2 6.3e-14, assemble-stride 6.6e-14.
No case failed: the kernels are right at every width, and k_bcn_assemble on its second trip.  Each test takes 0.02 .. 0.8 s,
assemble-stride 2.1 s.

THAT THE TESTS BITE: three arithmetic-only mutations, each on a scratch copy of the kernels (no index, bound, launch or memory
access changed), this file run on each:
  k_bcn_finish, the shuffle loop started at LG / 4           -> fails on the 13 cases with lgR >= 2, in gx alone (off by 2.7e-3
                                                                 on assemble-stride, 7.7e-3 .. 6.5e-2 on the others); passes on
                                                                 thin-r2 and lg2-r4 (lgR = 1)
  k_bn_prologue<LG, true>, lanes l >= 32 scaled by 1 + 1e-6  -> fails on both-64-r16, wide-rows-r1, both-64-shuffled-r16 and
                                                                 assemble-stride (lgA = 64; gx off by 5e-6 .. 2e-5); passes on
                                                                 the 11 cases with lgA <= 32
  k_bcn_assemble, wc written on its first trip only          -> assemble-stride alone fails, through Hv2 (4.2e-4) and Hv1
  (k < gridDim.x * 256)                                          (4.2e-4) under rho = 1; its gx, ys, gs, c, fx keep the figures
                                                                 of the clean run; the other 14 cases pass"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import nlpmodels  # noqa: E402
from fps_amd.device_qp import DeviceBandCoupledQuadNLP  # noqa: E402
import coupled_lane_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

SE, SIGMA = K.SE, K.SIGMA
BAR, BAR_JAC = 1e-9, 1e-13


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

    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).to(on)  # noqa: E731  (the cases' arrays are read-only: copies)
    gx, ys, gs = (torch.empty(k, dtype=torch.float64, device=on) for k in (qp.n, qp.m, qp.n))
    fx, rc = dev.objgrad(t(x), gx=gx, ys=ys, gs=gs, xk=t(xk))
    return fx, rc, gx.cpu().numpy(), ys.cpu().numpy(), gs.cpu().numpy()


@pytest.mark.parametrize("name", K.NAMES)
def test_every_entry_matches_the_exact_restatement(name):
    case, data = K.CASES[name], K.data(name)
    qp = data.qp
    assert K.lanes(data)[:3] == (case.lgA, case.lgT, case.lgR)
    x, xk, v = qp.x, qp.xhat, K.v_of(qp)
    for delta in K.deltas(name):
        want = K.expected(name, delta)
        dev = DeviceBandCoupledQuadNLP(data, sigma=SIGMA, rho=0.0, delta=delta, eta=0.0)
        info = dev.info()
        for k, val in case.band.items():
            assert info[k] == val, (k, info)
        assert info["border_rows"] == 0 and info["border_cols"] == 0
        c = np.empty(qp.m)
        assert dev.cons(x, c) == 0
        nobj = 0
        for (rho, eta), e in want.items():
            dev.rho, dev.eta = rho, eta
            fx, rc, gx, ys, gs = _objgrad(dev, x, xk)
            nobj += 1
            Hv2, Hv1 = np.empty(qp.n), np.empty(qp.n)
            assert rc == 0 and dev.hprod(v, Hv2, 2) == 0 and dev.hprod(v, Hv1, 1) == 0
            errs = {"gx": _rel(gx, e["gx"]), "ys": _rel(ys, e["ys"]), "gs": _rel(gs, e["gs"]), "c": _rel(c, e["c"]),
                    "Hv2": _rel(Hv2, e["Hv2"]), "Hv1": _rel(Hv1, e["Hv1"]), "fx": abs(fx - e["fx"]) / abs(e["fx"])}
            live = _rel(Hv1, Hv2)
            print(f"\nCOUPLED-LANES {name} lanes={case.lgA}/{case.lgT}/{case.lgR} delta={delta:.1e} rho={rho} eta={eta}: "
                  + " ".join(f"{k}={err:.2e}" for k, err in errs.items()) + f" Hv1-Hv2={live:.2e}")
            for k in ("gx", "ys", "gs", "c", "Hv2", "Hv1"):
                assert errs[k] < BAR, (k, errs[k])
            assert abs(fx - e["fx"]) <= BAR * abs(e["fx"])
            assert live > 1e-6                       # the Val(1)-only terms are live
            if name == K.STRIDE:                     # host and device arguments: the same bits
                import torch

                again = _objgrad(dev, x, xk, on=torch.device("cuda", 0))
                nobj += 1
                assert again[1] == 0
                for a, b in zip((fx, gx, ys, gs), (again[0],) + again[2:]):
                    assert np.array_equal(a, b)
        info = dev.info()
        assert info["factorizations"] == nobj and info["regularized_pivots"] == 0, info
        # the handle's values are J(x) now, terms included: fpsq_band_jac_mul multiplies with it
        J = nlpmodels.CoupledQuadConModel(data)._J(x)
        u, y, z = np.random.default_rng(2).standard_normal(qp.m), np.empty(qp.m), np.empty(qp.n)
        assert dev.jac_mul(0, 1.0, v, 0.0, y) == 0 and dev.jac_mul(1, 1.0, u, 0.0, z) == 0
        jac = {"J": _rel(y, J @ v), "J'": _rel(z, J.T @ u)}
        print(f"COUPLED-LANES {name} delta={delta:.1e} jac_mul: " + " ".join(f"{k}={err:.2e}" for k, err in jac.items()))
        assert jac["J"] < BAR_JAC and jac["J'"] < BAR_JAC
        dev.close()
