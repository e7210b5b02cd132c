"""fpsq_band_qp_objgrad_block / DeviceBandEqQP.objgrad_block: k penalty evaluations per call on the cached banded factor, 8 per
pass, column j on the model with its linear term replaced by D[j] and its right-hand side by B[j].

Yardsticks: per column, oracle.exact_qp_objgrad (diagonal Q) resp. tests/sparse_hessian_ref.py (sparse Q) on
dataclasses.replace(qp, d=D[j], b=B[j]), at the bars the single entry is held to in tests/test_gpu_band_qp.py and the block
entries in tests/test_gpu_band_block.py: max|a - b| / max|b| < 1e-9 per vector, |fx - fx_exact| <= 1e-9 |fx_exact|; and bitwise
equality wherever the interface promises it (a column -- fx included -- does not depend on k, on its position or on the other
columns; repeats; host and device arguments; null outputs).  Every call must return 0: a non-zero code is how a raised
error word of the sweeps shows.

Shapes: those of tests/test_gpu_band_block.py (m no multiple of 128, a reordered band, two elimination chains over 79
blocks, m a multiple of 128) and the smallest bordered one of tests/test_gpu_band_border.py; column counts 1, 3 (ragged
tile), 8 (exact tile), 11 (two tiles, the second ragged).  The references are computed once per column and shared."""
import copy
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
from fps_amd.device_qp import DeviceBandEqQP, DeviceBorderedBandEqQP  # noqa: E402
from sparse_hessian_ref import SparseHessianRef  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = 1e3
KMAX = 11
KS = (1, 3, 8, 11)
BAR = 1e-9
# name: (rho, eta, XK given)
VARIANTS = {"rho0-eta0": (0.0, 0.0, False), "rho1-eta.5-xk": (1.0, 0.5, True), "rho1-eta.5-xk-null": (1.0, 0.5, False)}
# name: (D given, B given)
FORMS = {"both": (True, True), "none": (False, False), "D-only": (True, False), "B-only": (False, True)}
OUTS = ("GX", "YS", "GS")


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _reordered(qp, order):
    """row p of the result = row order[p] of qp"""
    import scipy.sparse as sp

    A = sp.csr_matrix(qp.scipy_csr()[order])
    A.sort_indices()
    return dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy(),
                               b=qp.b[order])


def _small():
    return problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21)


def _bordered():
    """tests/test_gpu_band_border.py "mb640-s5-first-delta0": five mean-value rows in front of a 640-row band"""
    qp0 = problems.pde_control_like(n=3000, m=640, per_row=12, window=256, seed=5)
    qp = problems.with_border_rows(qp0, 5, kind="mean", seed=9)
    return _reordered(qp, np.concatenate([np.arange(qp0.m, qp.m), np.arange(qp0.m)]))


# name: (QP, delta, max_border, expected info)
BASES = {
    "small-delta0": (_small, 0.0, 0, {}),                                         # m = 400: not a multiple of 128
    "row-shuffled": (lambda: _reordered(_small(), np.random.default_rng(5).permutation(400)), 0.0, 0, {"reordered": 1}),
    "aug2dc": (lambda: problems.aug2dc_like(N=100), SE, 0, {"chains": 2, "nblocks": 79}),
    "m-multiple-of-128": (lambda: problems.pde_control_like(n=6000, m=640, per_row=24, window=512, seed=5), 1e-3, 0, {}),
    "bordered-s5": (_bordered, 0.0, 16, {"border_rows": 5, "nblocks": 5}),
}
MODELS = ("diag", "hw1", "hw8")


@functools.lru_cache(maxsize=None)
def _qp(case, model="diag"):
    qp = BASES[case][0]()
    return qp if model == "diag" else problems.with_sparse_hessian(qp, int(model[2:]), 11)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """X, D, B, XK: the (KMAX, .) blocks every test of a shape uses (read-only)"""
    qp = _qp(case)
    rng = np.random.default_rng(4321)
    blocks = (rng.standard_normal((KMAX, qp.n)), rng.standard_normal((KMAX, qp.n)), rng.standard_normal((KMAX, qp.m)),
              rng.standard_normal((KMAX, qp.n)))
    for a in blocks:
        a.setflags(write=False)
    return blocks


def _args(case, form, xk_given, cols=slice(None)):
    """the four input blocks of a call, restricted to `cols`; absent ones are None"""
    X, D, B, XK = _inputs(case)
    has_d, has_b = FORMS[form]
    pick = lambda a, on: np.ascontiguousarray(a[cols]) if on else None  # noqa: E731
    return pick(X, True), pick(D, has_d), pick(B, has_b), pick(XK, xk_given)


_EXACT = {}


def _exact(oracle, case, model, form, variant, j):
    """the exact evaluation of column j: dict(fx, gx, ys, gs), computed once"""
    key = (case, model, form, variant, j)
    if key not in _EXACT:
        qp, delta = _qp(case, model), BASES[case][1]
        rho, eta, xk_given = VARIANTS[variant]
        X, D, B, XK = _inputs(case)
        has_d, has_b = FORMS[form]
        qpj = dataclasses.replace(qp, d=D[j] if has_d else qp.d, b=B[j] if has_b else qp.b)
        xk = XK[j] if xk_given else None
        if model == "diag":
            e = oracle.exact_qp_objgrad(qpj, X[j], SIGMA, rho, delta, eta, xk)
        else:
            if ("lu", case, model) not in _EXACT:
                _EXACT["lu", case, model] = SparseHessianRef(qp, delta)        # K does not depend on d, b
            ref = copy.copy(_EXACT["lu", case, model])
            ref.qp = qpj
            e = ref.objgrad(X[j], SIGMA, rho, eta, xk)
        _EXACT[key] = {name: e[name] for name in ("fx", "gx", "ys", "gs")}
    return _EXACT[key]


def _device(case, model="diag", rho=1.0, eta=0.5):
    _, delta, border, want = BASES[case]
    if border:
        dev = DeviceBorderedBandEqQP(_qp(case, model), border=border, sigma=SIGMA, rho=rho, delta=delta, eta=eta)
    else:
        dev = DeviceBandEqQP(_qp(case, model), sigma=SIGMA, rho=rho, delta=delta, eta=eta)
    info = dev.info()
    for k, v in want.items():
        assert info[k] == v, (k, info)
    return dev


def _call(dev, X, D, B, XK, want=OUTS):
    """one block evaluation on host arrays; outputs not in `want` are null.  Returns (fx, {name: block})"""
    k, qp = X.shape[0], dev.qp
    size = {"GX": qp.n, "YS": qp.m, "GS": qp.n}
    out = {name: np.full((k, size[name]), np.nan) for name in want}
    fx, rc = dev.objgrad_block(X, XK=XK, D=D, B=B, **out)
    assert rc == 0 and fx.shape == (k,)
    return fx, out


def _flat(fx, out):
    """fx and the three output blocks side by side: row j = everything column j produced"""
    return np.concatenate([fx[:, None], out["GX"], out["YS"], out["GS"]], axis=1)


def _check(got, exact, what):
    """the bars of this file on one column; returns the four figures"""
    fx, out, j = got
    errs = {"gx": _rel(out["GX"][j], exact["gx"]), "ys": _rel(out["YS"][j], exact["ys"]), "gs": _rel(out["GS"][j], exact["gs"]),
            "fx": abs(fx[j] - exact["fx"]) / abs(exact["fx"])}
    assert errs["gx"] < BAR and errs["ys"] < BAR and errs["gs"] < BAR, (what, errs)
    assert abs(fx[j] - exact["fx"]) <= 1e-9 * abs(exact["fx"]), (what, errs)
    return errs


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(BASES))
def test_block_objgrad_matches_the_exact_evaluation_per_column(oracle, case, model, variant):
    rho, eta, xk_given = VARIANTS[variant]
    dev = _device(case, model, rho, eta)
    # D and B both given at every column count; the model's own d and / or b on a ragged tile
    for form, ks in (("both", KS), ("none", (3,)), ("D-only", (3,)), ("B-only", (3,))):
        for k in ks:
            fx, out = _call(dev, *_args(case, form, xk_given, slice(0, k)))
            worst = {}
            for j in range(k):
                errs = _check((fx, out, j), _exact(oracle, case, model, form, variant, j), (form, k, j))
                worst = {name: max(worst.get(name, 0.0), v) for name, v in errs.items()}
            print(f"\n{case} {model} {variant} {form} k={k}: max rel err " + " ".join(f"{a}={v:.2e}" for a, v in worst.items()))
    assert dev.info()["factorizations"] == 1
    dev.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(BASES))
def test_a_column_does_not_depend_on_k_position_repeats_or_the_other_columns(case, model):
    blocks = _args(case, "both", True)
    dev = _device(case, model)

    def run(blocks):
        return _flat(*_call(dev, *(np.ascontiguousarray(a) for a in blocks)))

    full = run(blocks)
    assert np.all(np.isfinite(full))
    assert np.array_equal(run(blocks), full)                                      # a second identical call
    perm = np.random.default_rng(7).permutation(KMAX)
    assert not np.array_equal(perm, np.arange(KMAX))
    assert np.array_equal(run([a[perm] for a in blocks]), full[perm])             # a column permutation
    rng = np.random.default_rng(8)
    with np.errstate(all="ignore"):
        for j in range(KMAX):
            assert np.array_equal(run([a[j:j + 1] for a in blocks])[0], full[j]), j      # k = 1
            noise = [1e300 * rng.standard_normal(a.shape) for a in blocks]
            for z, a in zip(noise, blocks):
                z[j] = a[j]
            assert np.array_equal(run(noise)[j], full[j]), j                     # every other column: 1e300-scaled noise
    dev.close()


@pytest.mark.parametrize("model", ("diag", "hw8"))
def test_host_and_device_blocks_give_the_same_bits(model):
    import torch

    case = "aug2dc"
    blocks = _args(case, "both", True)
    on = torch.device("cuda", 0)
    dev = _device(case, model)
    hfx, hout = _call(dev, *blocks)
    # Device tensors with torch work queued in front of them on torch's CURRENT stream, which objgrad_block registers: no
    # synchronisation between the producers and the call.  (No stream of the test's own: a torch stream lives as long as the
    # process and would take a share of the hardware queues from every test that runs after this one.)
    load = torch.zeros(1 << 24, dtype=torch.float64, device=on)
    for _ in range(16):
        load = load * 0.5 + 1.0
    halves = [torch.from_numpy(0.5 * a).to(on, non_blocking=True) for a in blocks]
    Xd, Dd, Bd, XKd = (h + h for h in halves)              # (exact: the blocks again, produced behind the load)
    outs = {name: torch.full(hout[name].shape, float("nan"), dtype=torch.float64, device=on) for name in OUTS}
    fx, rc = dev.objgrad_block(Xd, XK=XKd, D=Dd, B=Bd, **outs)
    assert rc == 0 and np.array_equal(fx, hfx)
    for name in OUTS:
        assert np.array_equal(outs[name].cpu().numpy(), hout[name]), name
    mixed = {name: np.full(hout[name].shape, np.nan) for name in OUTS}      # inputs on the device, outputs on the host
    fx, rc = dev.objgrad_block(Xd, XK=XKd, D=Dd, B=Bd, **mixed)
    assert rc == 0 and np.array_equal(fx, hfx)
    for name in OUTS:
        assert np.array_equal(mixed[name], hout[name]), name
    assert np.array_equal(Xd.cpu().numpy(), blocks[0])
    dev.close()


@pytest.mark.parametrize("case", list(BASES))
def test_block_and_single_entries_agree_through_the_exact_reference(oracle, case):
    """The matrix-core sweep sums in another order than the single-vector sweep: the two are not bitwise equal and nothing is
    asserted about their difference (printed) but what follows from both being within the bars of the exact reference."""
    variant = "rho1-eta.5-xk"
    X, _, _, XK = _args(case, "none", True, slice(0, 3))
    dev = _device(case)
    fx, out = _call(dev, X, None, None, XK)
    sfx, sout = np.empty(3), {name: np.empty_like(out[name]) for name in OUTS}
    for j in range(3):
        sfx[j], rc = dev.objgrad(X[j], gx=sout["GX"][j], ys=sout["YS"][j], gs=sout["GS"][j], xk=XK[j])
        assert rc == 0
    diff = {name: max(_rel(out[name][j], sout[name][j]) for j in range(3)) for name in OUTS}
    diff["fx"] = float(np.max(np.abs(fx - sfx) / np.abs(sfx)))
    print(f"\n{case}: block against single, max rel diff " + " ".join(f"{a}={v:.2e}" for a, v in diff.items()))
    for j in range(3):
        e = _exact(oracle, case, "diag", "none", variant, j)
        _check((fx, out, j), e, ("block", j))
        _check((sfx, sout, j), e, ("single", j))
    dev.close()


def test_null_outputs_arguments_and_state():
    case = "small-delta0"
    qp, delta = _qp(case), BASES[case][1]
    n, m = qp.n, qp.m
    X, D, B, XK = _args(case, "both", True, slice(0, 3))
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
    lib, h, q = dev._lib, dev._h, dev._q
    fx = np.full(3, np.nan)
    GX, YS, GS = np.empty((3, n)), np.empty((3, m)), np.empty((3, n))

    def entry(k, x, fxp, gx, d=D.ctypes.data):
        return lib.fpsq_band_qp_objgrad_block(h, q, k, x, d, B.ctypes.data, SIGMA, 1.0, 0.5, XK.ctypes.data, fxp, gx,
                                              YS.ctypes.data, GS.ctypes.data)

    # before any factorisation
    assert entry(3, X.ctypes.data, fx.ctypes.data, GX.ctypes.data) == -3
    assert b"factorisation" in lib.fpsq_band_last_error(h)
    gfx, good = _call(dev, X, D, B, XK)
    assert dev.info()["factorizations"] == 1
    # null outputs in every combination: the others do not change a bit, nor does fx
    for want in ((), ("GX",), ("YS",), ("GS",), ("GX", "YS"), ("GX", "GS"), ("YS", "GS")):
        pfx, part = _call(dev, X, D, B, XK, want=want)
        assert np.array_equal(pfx, gfx), want
        for name in want:
            assert np.array_equal(part[name], good[name]), (want, name)
    # k = 0, a null X, a null fx
    assert entry(0, X.ctypes.data, fx.ctypes.data, GX.ctypes.data) == -1
    assert entry(3, None, fx.ctypes.data, GX.ctypes.data) == -1
    assert entry(3, X.ctypes.data, None, GX.ctypes.data) == -1
    # GX starts inside X, inside D
    buf = np.zeros(6 * n)
    buf[:3 * n] = X.ravel()
    for shift in (0, n, 2 * n + 1):
        assert entry(3, buf.ctypes.data, fx.ctypes.data, buf.ctypes.data + 8 * shift) == -1
        assert b"overlap" in lib.fpsq_band_last_error(h)
        assert entry(3, X.ctypes.data, fx.ctypes.data, buf.ctypes.data + 8 * shift, d=buf.ctypes.data) == -1
    assert np.array_equal(buf[:3 * n], X.ravel())
    assert lib.fpsq_band_qp_objgrad_block(h, q, 3, X.ctypes.data, None, None, SIGMA, 1.0, 0.5, None, fx.ctypes.data,
                                          GX.ctypes.data, None, GX.ctypes.data + 8 * n) == -1          # GS inside GX
    assert b"overlap" in lib.fpsq_band_last_error(h)
    # ... and right behind X: fine
    assert entry(3, buf.ctypes.data, fx.ctypes.data, buf.ctypes.data + 8 * 3 * n) == 0
    assert np.array_equal(fx, gfx) and np.array_equal(buf[3 * n:].reshape(3, n), good["GX"])
    assert np.array_equal(YS, good["YS"]) and np.array_equal(GS, good["GS"])
    # a model of another handle
    other = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
    assert lib.fpsq_band_qp_objgrad_block(h, other._q, 3, X.ctypes.data, None, None, SIGMA, 1.0, 0.5, None, fx.ctypes.data,
                                          None, None, None) == -1
    other.close()
    # the handle stays usable and repeatable
    again, out = _call(dev, X, D, B, XK)
    assert np.array_equal(again, gfx) and all(np.array_equal(out[name], good[name]) for name in OUTS)
    dev.close()


@pytest.mark.parametrize("case", ("small-delta0", "bordered-s5"))
def test_the_python_method_on_device_tensors_and_a_stale_factor(oracle, case):
    import torch

    on = torch.device("cuda", 0)
    qp = _qp(case)
    blocks = _args(case, "both", True, slice(0, 3))
    dev = _device(case)
    assert isinstance(dev, DeviceBorderedBandEqQP) == (case == "bordered-s5")
    X, D, B, XK = (torch.tensor(a, device=on) for a in blocks)
    outs = {"GX": torch.empty(3, qp.n, dtype=torch.float64, device=on), "YS": torch.empty(3, qp.m, dtype=torch.float64, device=on),
            "GS": torch.empty(3, qp.n, dtype=torch.float64, device=on)}

    def run():
        fx, rc = dev.objgrad_block(X, XK=XK, D=D, B=B, **outs)
        assert rc == 0 and isinstance(fx, np.ndarray) and fx.shape == (3,)
        return fx, {name: t.cpu().numpy() for name, t in outs.items()}

    fx, out = run()
    for j in range(3):
        _check((fx, out, j), _exact(oracle, case, "diag", "both", "rho1-eta.5-xk", j), j)
    run()
    assert dev.info()["factorizations"] == 1
    dev.set_delta(1e-3)                                   # the factor is stale: rebuilt once, at the next evaluation
    fx, out = run()
    run()
    assert dev.info()["factorizations"] == 2
    e = oracle.exact_qp_objgrad(dataclasses.replace(qp, d=blocks[1][0], b=blocks[2][0]), blocks[0][0], SIGMA, 1.0, 1e-3, 0.5,
                                blocks[3][0])
    _check((fx, out, 0), e, "delta = 1e-3")
    # the guards of the block helper
    with pytest.raises(ValueError):
        dev.objgrad_block(X, D=torch.zeros(2, qp.n, dtype=torch.float64, device=on))
    with pytest.raises(ValueError):
        dev.objgrad_block(X, B=np.zeros((3, qp.n)))
    with pytest.raises(ValueError):
        dev.objgrad_block(blocks[0].astype(np.float32))
    dev.close()


def test_a_diagonal_and_a_sparse_model_on_one_handle_do_not_disturb_each_other(oracle):
    case = "small-delta0"
    qp, qs = _qp(case), _qp(case, "hw8")
    n, m = qp.n, qp.m
    X, D, B, XK = _args(case, "both", True, slice(0, 3))
    dev = _device(case)
    lib, h = dev._lib, dev._h
    qsp = C.c_void_p()
    hrp, hci = np.ascontiguousarray(qs.hess_rowptr, dtype=np.int32), np.ascontiguousarray(qs.hess_colind, dtype=np.int32)
    assert lib.fpsq_band_qp_create_csr(h, hrp.ctypes.data, hci.ctypes.data, qs.hess_vals.ctypes.data, qs.d.ctypes.data,
                                       qs.b.ctypes.data, C.byref(qsp)) == 0
    assert dev._factor() == 0

    def run(model):
        fx, out = np.full(3, np.nan), {"GX": np.full((3, n), np.nan), "YS": np.full((3, m), np.nan), "GS": np.full((3, n), np.nan)}
        assert lib.fpsq_band_qp_objgrad_block(h, model, 3, X.ctypes.data, D.ctypes.data, B.ctypes.data, SIGMA, 1.0, 0.5,
                                              XK.ctypes.data, fx.ctypes.data, out["GX"].ctypes.data, out["YS"].ctypes.data,
                                              out["GS"].ctypes.data) == 0
        return fx, out

    first = {"diag": run(dev._q), "hw8": run(qsp)}
    for name, model in (("diag", dev._q), ("hw8", qsp), ("hw8", qsp), ("diag", dev._q)):
        fx, out = run(model)
        assert np.array_equal(fx, first[name][0]), name
        for o in OUTS:
            assert np.array_equal(out[o], first[name][1][o]), (name, o)
    assert not np.array_equal(first["diag"][1]["GX"], first["hw8"][1]["GX"])
    for name in ("diag", "hw8"):
        for j in range(3):
            _check((*first[name], j), _exact(oracle, case, name, "both", "rho1-eta.5-xk", j), (name, j))
    lib.fpsq_band_qp_destroy(qsp)
    dev.close()
