"""Block entries on the cached banded factor: fpsq_band_solve_two_least_squares_block and fpsq_band_qp_hprod_block (k vectors
per call, 8 per pass over the factor on the fp64 matrix cores), DeviceBandEqQP.solve_two_least_squares_block / hprod_block.

Yardsticks: the exact KKT solve per column (oracle.exact_two_least_squares / exact_qp_hprod; tests/sparse_hessian_ref.py for
a sparse objective Hessian) at the bar tests/test_gpu_band_qp.py holds this factor to, max|a - b| / max|b| < 1e-9 per vector;
and bitwise equality wherever the interface promises it (a column does not depend on k, on its position or on the other
columns; host and device arguments; repeats; hessian_approx 1 and 2).  Every call must return 0: a non-zero code is how a
raised error word of the sweeps shows.

Shapes: the smallest that exercise each addressing case (m no multiple of 128, a reordered band, two elimination chains
over 79 blocks, m a multiple of 128); column counts 1, 3 (ragged tile), 8 (exact tile), 11 (two tiles, the second ragged)."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import problems  # noqa: E402
from fps_amd.device_qp import DeviceBandEqQP  # noqa: E402
from sparse_hessian_ref import SparseHessianRef  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = 1e3
KMAX = 11
KS = (1, 3, 8, 11)
RHO_ETA = ((0.0, 0.0), (1.0, 0.5))
BAR = 1e-9


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _shuffled(qp, seed):
    """the same QP with its constraint rows in a random order (a full natural band: the symbolic phase reorders)"""
    import scipy.sparse as sp

    perm = np.random.default_rng(seed).permutation(qp.m)
    A = sp.csr_matrix(qp.scipy_csr()[perm])
    A.sort_indices()
    return dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy(),
                               b=qp.b[perm])


def _small():
    return problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21)


BASES = {
    "small-delta0": (_small, 0.0, {}),                                            # m = 400: not a multiple of 128
    "row-shuffled": (lambda: _shuffled(_small(), 5), 0.0, {"reordered": 1}),
    "aug2dc": (lambda: problems.aug2dc_like(N=100), SE, {"chains": 2, "nblocks": 79}),
    "m-multiple-of-128": (lambda: problems.pde_control_like(n=6000, m=640, per_row=24, window=512, seed=5), 1e-3, {}),
}
MODELS = ("diag", "hw1", "hw8")


@functools.lru_cache(maxsize=None)
def _qp(case, model="diag"):
    qp = BASES[case][0]()
    return qp if model == "diag" else problems.with_sparse_hessian(qp, int(model[2:]), 11)


@functools.lru_cache(maxsize=None)
def _blocks(case):
    """the KMAX x n blocks every test of a shape uses (read-only)"""
    qp = _qp(case)
    rng = np.random.default_rng(1234)
    V, W = rng.standard_normal((KMAX, qp.n)), rng.standard_normal((KMAX, qp.n))
    V.setflags(write=False)
    W.setflags(write=False)
    return V, W


_EXACT = {}


def _exact_solve(oracle, case):
    """oracle.exact_two_least_squares per column of the shape's blocks, computed once: (p1, q1, p2, q2) as (KMAX, .) arrays"""
    if ("solve", case) not in _EXACT:
        qp, delta = _qp(case), BASES[case][1]
        V, W = _blocks(case)
        A = qp.scipy_csr()
        cols = [oracle.exact_two_least_squares(A, delta, V[j], W[j]) for j in range(KMAX)]
        _EXACT["solve", case] = tuple(np.stack([c[i] for c in cols]) for i in range(4))
    return _EXACT["solve", case]


def _exact_hprod(oracle, case, model, rho, eta):
    """the exact Hessian products of the shape's V, (KMAX, n), computed once per model and (rho, eta)"""
    key = ("hprod", case, model, rho, eta)
    if key not in _EXACT:
        qp, delta = _qp(case, model), BASES[case][1]
        V, _ = _blocks(case)
        if model == "diag":
            _EXACT[key] = np.stack([oracle.exact_qp_hprod(qp, V[j], SIGMA, rho, delta, eta) for j in range(KMAX)])
        else:
            if ("ref", case, model) not in _EXACT:
                _EXACT["ref", case, model] = SparseHessianRef(qp, delta)
            ref = _EXACT["ref", case, model]
            _EXACT[key] = np.stack([ref.hprod(V[j], SIGMA, rho, eta) for j in range(KMAX)])
    return _EXACT[key]


def _device(case, model="diag", rho=1.0, eta=0.5):
    dev = DeviceBandEqQP(_qp(case, model), sigma=SIGMA, rho=rho, delta=BASES[case][1], eta=eta)
    info = dev.info()
    for k, v in BASES[case][2].items():
        assert info[k] == v, (k, info)
    return dev


def _solve(dev, R1, R2, want=("p1", "q1", "p2", "q2")):
    """one block solve on host arrays; outputs not in `want` are null"""
    k, qp = R1.shape[0], dev.qp
    size = {"p1": qp.n, "q1": qp.m, "p2": qp.n, "q2": qp.m}
    out = {name: np.full((k, size[name]), np.nan) for name in want}
    assert dev.solve_two_least_squares_block(np.ascontiguousarray(R1), np.ascontiguousarray(R2), **out) == 0
    return out


def _hprod(dev, V, approx=2):
    HV = np.full(V.shape, np.nan)
    assert dev.hprod_block(np.ascontiguousarray(V), HV, approx) == 0
    return HV


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", list(BASES))
def test_block_solve_matches_the_exact_kkt_solve_per_column(oracle, case, k):
    exact = dict(zip(("p1", "q1", "p2", "q2"), _exact_solve(oracle, case)))
    V, W = _blocks(case)
    dev = _device(case)
    got = _solve(dev, V[:k], W[:k])
    for name in ("p1", "q1", "p2", "q2"):
        errs = [_rel(got[name][j], exact[name][j]) for j in range(k)]
        print(f"\n{case} k={k} {name}: max rel err {max(errs):.3e}")
        assert max(errs) < BAR, (name, errs)
    # some outputs null: the others do not change a bit
    for want in (("p1",), ("q2",), ("q1", "p2"), ("p1", "q1", "p2"), ()):
        part = _solve(dev, V[:k], W[:k], want=want)
        for name in want:
            assert np.array_equal(part[name], got[name]), (want, name)
    assert dev.info()["factorizations"] == 1
    dev.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(BASES))
def test_block_hprod_matches_the_exact_evaluation(oracle, case, model):
    V, _ = _blocks(case)
    dev = _device(case, model)
    for rho, eta in RHO_ETA:
        dev.rho, dev.eta = rho, eta
        exact = _exact_hprod(oracle, case, model, rho, eta)
        for k in KS:
            H2, H1 = _hprod(dev, V[:k], 2), _hprod(dev, V[:k], 1)
            errs = [_rel(H2[j], exact[j]) for j in range(k)]
            print(f"\n{case} {model} rho={rho} eta={eta} k={k}: max rel err {max(errs):.3e}")
            assert max(errs) < BAR, errs
            assert np.array_equal(H1, H2)      # Val(1): the extra terms vanish identically for linear constraints
    assert dev.info()["factorizations"] == 1
    dev.close()


@pytest.mark.parametrize("entry", ("solve",) + MODELS)
@pytest.mark.parametrize("case", list(BASES))
def test_a_column_does_not_depend_on_k_position_repeats_or_the_other_columns(case, entry):
    V, W = _blocks(case)
    dev = _device(case, "diag" if entry == "solve" else entry)
    if entry == "solve":
        def run(A, B):
            o = _solve(dev, A, B)
            return np.concatenate([o["p1"], o["q1"], o["p2"], o["q2"]], axis=1)
    else:
        def run(A, B):
            return _hprod(dev, A)
    full = run(V, W)
    assert np.all(np.isfinite(full))
    assert np.array_equal(run(V, W), full)                                    # a second identical call
    perm = np.random.default_rng(7).permutation(KMAX)
    assert not np.array_equal(perm, np.arange(KMAX))
    assert np.array_equal(run(V[perm], W[perm]), full[perm])                  # a column permutation
    rng = np.random.default_rng(8)
    with np.errstate(all="ignore"):
        for j in range(KMAX):
            assert np.array_equal(run(V[j:j + 1], W[j:j + 1])[0], full[j]), j   # k = 1
            N1, N2 = 1e300 * rng.standard_normal(V.shape), 1e300 * rng.standard_normal(V.shape)
            N1[j], N2[j] = V[j], W[j]
            assert np.array_equal(run(N1, N2)[j], full[j]), j                # every other column: 1e300-scaled noise
    dev.close()


@pytest.mark.parametrize("model", ("diag", "hw8"))
def test_host_and_device_blocks_give_the_same_bits(model):
    import torch

    case = "aug2dc"
    V, W = _blocks(case)
    on = torch.device("cuda", 0)
    dev = _device(case, model)
    host = _hprod(dev, V)
    hsolve = _solve(dev, V, W)
    # Device tensors with torch work queued in front of them on torch's CURRENT stream, which hprod_block registers: no
    # synchronisation between the producers and the call.  (No stream of the test's own: a torch stream lives as long as the
    # process and would take a share of the hardware queues from every test that runs after this one.)
    load = torch.zeros(1 << 24, dtype=torch.float64, device=on)
    for _ in range(16):
        load = load * 0.5 + 1.0
    half_v, half_w = (torch.from_numpy(0.5 * a).to(on, non_blocking=True) for a in (V, W))
    Vd, Wd = half_v + half_v, half_w + half_w          # (exact: V, W again, produced behind the load)
    Hd = torch.full(V.shape, float("nan"), dtype=torch.float64, device=on)
    assert dev.hprod_block(Vd, Hd) == 0
    outs = {name: torch.full((KMAX, size), float("nan"), dtype=torch.float64, device=on)
            for name, size in (("p1", dev.qp.n), ("q1", dev.qp.m), ("p2", dev.qp.n), ("q2", dev.qp.m))}
    assert dev.solve_two_least_squares_block(Vd, Wd, **outs) == 0
    Hmixed = np.full(V.shape, np.nan)                  # V on the device, HV on the host
    assert dev.hprod_block(Vd, Hmixed) == 0
    assert np.array_equal(Vd.cpu().numpy(), V)
    assert np.array_equal(Hd.cpu().numpy(), host)
    assert np.array_equal(Hmixed, host)
    for name in outs:
        assert np.array_equal(outs[name].cpu().numpy(), hsolve[name]), name
    dev.close()


@pytest.mark.parametrize("case", list(BASES))
def test_block_and_single_vector_entries_agree_through_the_exact_reference(oracle, case):
    """The matrix-core sweep sums in another order than the single-vector sweep: the two are not bitwise equal and nothing is
    asserted about their difference (printed) but what follows from both being within the bar of the exact reference."""
    V, _ = _blocks(case)
    dev = _device(case)
    exact = _exact_hprod(oracle, case, "diag", 1.0, 0.5)
    block = _hprod(dev, V)
    single = np.empty_like(block)
    for j in range(KMAX):
        assert dev.hprod(np.ascontiguousarray(V[j]), single[j]) == 0
    diff = max(_rel(block[j], single[j]) for j in range(KMAX))
    eb, es = (max(_rel(x[j], exact[j]) for j in range(KMAX)) for x in (block, single))
    print(f"\n{case}: block against single max rel diff {diff:.3e}; against exact: block {eb:.3e}, single {es:.3e}")
    assert eb < BAR and es < BAR
    dev.close()


def test_arguments_and_state():
    case = "small-delta0"
    qp, delta = _qp(case), BASES[case][1]
    V, W = _blocks(case)
    V3, W3 = np.ascontiguousarray(V[:3]), np.ascontiguousarray(W[:3])
    n, m = qp.n, qp.m
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
    lib, h, q = dev._lib, dev._h, dev._q
    H = np.empty((3, n))
    outs = [np.empty((3, s)) for s in (n, m, n, m)]
    # before any factorisation
    assert lib.fpsq_band_qp_hprod_block(h, q, 3, V3.ctypes.data, SIGMA, 1.0, 0.5, 2, H.ctypes.data) == -3
    assert lib.fpsq_band_solve_two_least_squares_block(h, 3, V3.ctypes.data, W3.ctypes.data,
                                                       *[o.ctypes.data for o in outs]) == -3
    assert b"factorisation" in lib.fpsq_band_last_error(h)
    assert dev.hprod_block(V3, H) == 0 and dev.info()["factorizations"] == 1
    good = H.copy()
    # k = 0, overlapping V / HV, hessian_approx = 3, null blocks
    assert lib.fpsq_band_qp_hprod_block(h, q, 0, V3.ctypes.data, SIGMA, 1.0, 0.5, 2, H.ctypes.data) == -1
    assert lib.fpsq_band_solve_two_least_squares_block(h, 0, V3.ctypes.data, W3.ctypes.data,
                                                       *[o.ctypes.data for o in outs]) == -1
    buf = np.zeros(6 * n)
    buf[:3 * n] = V3.ravel()
    for shift in (0, n, 2 * n + 1):      # HV starts inside V
        assert lib.fpsq_band_qp_hprod_block(h, q, 3, buf.ctypes.data, SIGMA, 1.0, 0.5, 2, buf.ctypes.data + 8 * shift) == -1
        assert b"overlap" in lib.fpsq_band_last_error(h)
    assert np.array_equal(buf[:3 * n], V3.ravel())
    # ... and right behind it: fine
    assert lib.fpsq_band_qp_hprod_block(h, q, 3, buf.ctypes.data, SIGMA, 1.0, 0.5, 2, buf.ctypes.data + 8 * 3 * n) == 0
    assert np.array_equal(buf[3 * n:].reshape(3, n), good)
    assert lib.fpsq_band_qp_hprod_block(h, q, 3, V3.ctypes.data, SIGMA, 1.0, 0.5, 3, H.ctypes.data) == -1
    assert b"hessian_approx" in lib.fpsq_band_last_error(h)
    assert lib.fpsq_band_qp_hprod_block(h, q, 3, None, SIGMA, 1.0, 0.5, 2, H.ctypes.data) == -1
    assert lib.fpsq_band_qp_hprod_block(h, q, 3, V3.ctypes.data, SIGMA, 1.0, 0.5, 2, None) == -1
    assert lib.fpsq_band_solve_two_least_squares_block(h, 3, None, W3.ctypes.data, *[o.ctypes.data for o in outs]) == -1
    # the handle stays usable and repeatable
    assert dev.hprod_block(V3, H) == 0 and np.array_equal(H, good)
    dev.close()


def test_set_delta_costs_one_factorisation_and_the_result_follows(oracle):
    case = "small-delta0"
    qp = _qp(case)
    V, _ = _blocks(case)
    V3 = np.ascontiguousarray(V[:3])
    dev = _device(case)
    _hprod(dev, V3)
    _hprod(dev, V3)
    assert dev.info()["factorizations"] == 1
    dev.set_delta(1e-3)
    H = _hprod(dev, V3)
    out = _solve(dev, V3, V3)
    assert dev.info()["factorizations"] == 2
    for j in range(3):
        assert _rel(H[j], oracle.exact_qp_hprod(qp, V3[j], SIGMA, 1.0, 1e-3, 0.5)) < BAR
    e = oracle.exact_two_least_squares(qp.scipy_csr(), 1e-3, V3[0], V3[0])
    assert _rel(out["p1"][0], e[0]) < BAR and _rel(out["q2"][0], e[3]) < BAR
    dev.close()


@pytest.mark.parametrize("model", ("diag", "hw8"))
def test_block_calls_leave_the_single_vector_entries_bitwise_unchanged(model):
    case = "aug2dc"
    qp = _qp(case, model)
    V, W = _blocks(case)
    x, xk = qp.point(2), qp.xhat

    def single(dev):
        gx, ys, gs, Hv = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.n)
        fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xk)
        assert rc == 0 and dev.hprod(np.ascontiguousarray(V[0]), Hv) == 0
        return fx, gx, ys, gs, Hv

    fresh = _device(case, model)
    want = single(fresh)
    fresh.close()
    dev = _device(case, model)
    _hprod(dev, V)
    _solve(dev, V, W)
    first = single(dev)
    _hprod(dev, V[:3])
    second = single(dev)
    for got in (first, second):
        assert got[0] == want[0]
        for a, b in zip(got[1:], want[1:]):
            assert np.array_equal(a, b)
    dev.close()


def test_python_guards_refuse_a_wrong_shape_dtype_or_layout():
    import torch

    case = "small-delta0"
    qp = _qp(case)
    n, m = qp.n, qp.m
    dev = _device(case)
    V = np.ascontiguousarray(_blocks(case)[0][:3])
    H = np.empty((3, n))
    bad = [
        (np.zeros(n), H),                                    # one dimension
        (np.zeros((3, n + 1)), np.empty((3, n + 1))),        # wrong length
        (V, np.empty((2, n))),                               # k differs
        (V.astype(np.float32), H),                           # dtype
        (V, np.empty((3, n), dtype=np.float32)),
        (np.zeros((n, 3)).T, H),                             # not C-contiguous
        (V, np.empty((3, 2 * n))[:, ::2]),
        (torch.zeros(3, n, dtype=torch.float32), H),
        (torch.zeros(n, 3, dtype=torch.float64).T, H),
        (V.tolist(), H),
        (np.zeros((0, n)), np.zeros((0, n))),                # k = 0
    ]
    for a, b in bad:
        with pytest.raises(ValueError):
            dev.hprod_block(a, b)
    with pytest.raises(ValueError):
        dev.solve_two_least_squares_block(V, np.zeros((3, m)), p1=H)            # rhs2 is an n-block
    with pytest.raises(ValueError):
        dev.solve_two_least_squares_block(V, V, q1=np.empty((3, n)))            # q1 is an m-block
    with pytest.raises(ValueError):
        dev.solve_two_least_squares_block(V, V, p2=np.empty((3, 2 * n))[:, ::2])
    with pytest.raises(ValueError):
        dev.solve_two_least_squares_block(None, V)
    assert dev.info()["factorizations"] == 0                 # refused before the library was called
    assert dev.hprod_block(V, H) == 0
    dev.close()
