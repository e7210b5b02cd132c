"""The cases of tests/coupled_lane_cases.py as far as they can be checked without a GPU: the three lane groups of every case
recomputed and held to the pinned literals, that together they reach every width on every side, that the term rule gives valid
terms with xhat feasible, that the couplings matter and J(x) is well posed on each case, and that the yardstick the GPU test
(tests/test_gpu_coupled_lane_groups.py) compares with solves its own system."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import nlpmodels, problems, qdsolver  # noqa: E402
import coupled_cases as cc  # noqa: E402
import coupled_lane_cases as K  # noqa: E402
import lane_group_cases as L  # noqa: E402
from coupled_nlp_model import build_lists  # noqa: E402
from sepquad_ref import SepQuadRef  # noqa: E402

SE = K.SE
LIST_TERMS = 20000    # build_lists walks the terms in Python: above this many it is given the terms of every step-th row


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("name", K.NAMES)
def test_the_lane_groups_are_the_pinned_ones(name):
    c, d = K.CASES[name], K.data(name)
    lgA, lgT, lgR, snz, longest = K.lanes(d)
    print(f"\n{name}: lgA={lgA} lgT={lgT} lgR={lgR} nnz(S)={snz} terms={d.nterms} longest row of S={longest}")
    assert (lgA, lgT, lgR) == (c.lgA, c.lgT, c.lgR)
    assert (snz, d.nterms, longest) == (c.snz, c.nterms, c.longest)
    if c.base is not None:
        assert (c.lgA, c.lgT) == (L.CASES[c.base].lgA, L.CASES[c.base].lgT) and c.band is L.CASES[c.base].band


def test_the_cases_reach_every_width_on_every_side():
    C = K.CASES
    assert {c.lgA for c in C.values()} == set(K.WIDTHS)
    assert {c.lgT for c in C.values()} == set(K.WIDTHS)
    assert {c.lgR for c in C.values()} == set(K.WIDTHS)
    # the terms' rows through the permutation of a reordered handle at 32 lanes and at 64
    assert {(c.lgA, c.lgT, c.lgR) for c in C.values() if c.band["reordered"]} == {(64, 64, 64), (32, 32, 16)}
    # rows without a term next to rows with many
    for name in ("thin-r2", "ragged-r2", "ragged-shuffled-r2"):
        d = K.data(name)
        per_row = np.bincount(d.t_row, minlength=d.qp.m)
        assert per_row.min() == 0 and np.all((per_row == 0) == (np.diff(d.qp.rowptr) == 1)), name
    assert np.bincount(K.data("ragged-r2").t_row).max() == 397
    # k_bcn_assemble: a thread per entry of S, the flat grid capped at 4096 workgroups of 256 -- a second trip on one case only
    s = C[K.STRIDE]
    assert s.snz > L.MAX_GRID_FLAT * 256 and (s.snz + 255) // 256 == 6501 and s.longest > 16 * s.lgR
    assert all(c.snz <= L.MAX_GRID_FLAT * 256 for k, c in C.items() if k != K.STRIDE)
    # small shapes: the row kernels' own second trips are tests/coupled_cases.py STRIDE's
    for name in K.NAMES:
        qp = K.data(name).qp
        assert max(qp.n, qp.m) <= 3600 and L.tiles(max(qp.n, 128 * ((qp.m + 127) // 128)), 1) <= L.MAX_GRID, name
    assert set(K.DELTA0) <= set(K.NAMES) and len(K.DELTA0) == 3


def test_the_symbolic_phase_takes_assemble_stride():
    """the other cases are shapes of tests/lane_group_cases.py, which tests/test_lane_groups_cpu.py puts through the analysis"""
    qp = K.data(K.STRIDE).qp
    assert (qp.n, qp.m, qp.nnz) == (2048, 160, 25600) and np.all(np.diff(qp.rowptr) == 160)
    info = qdsolver.band_analysis(nlpmodels.EqQPModel(qp))
    assert info is not None
    assert {k: info[k] for k in K.CASES[K.STRIDE].band} == K.CASES[K.STRIDE].band
    assert info["border_rows"] == 0 and info["border_cols"] == 0


@pytest.mark.parametrize("name", K.NAMES)
def test_the_term_rule_gives_valid_terms(name):
    c, d = K.CASES[name], K.data(name)
    qp = d.qp
    n, m = qp.n, qp.m
    assert d.t_row.dtype == np.int32 and d.t_j.dtype == np.int32 and d.t_k.dtype == np.int32 and d.t_w.dtype == np.float64
    assert np.array_equal(d.hvals, problems.with_quadratic_constraints(qp, K.CURV, K.SEED).hvals)
    assert np.abs(nlpmodels.CoupledQuadConModel(d).cons(qp.xhat)).max() < 1e-12          # xhat is feasible
    t_row, t_j, t_k = (a.astype(np.int64) for a in (d.t_row, d.t_j, d.t_k))
    # both columns of a term are entries of its row; j < k (the entries of a row ascend); no pair twice in a row; the order
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(qp.rowptr))
    pattern = rows * n + qp.colind
    assert np.all(np.isin(t_row * n + t_j, pattern)) and np.all(np.isin(t_row * n + t_k, pattern))
    assert np.all(t_j < t_k)
    key = (t_row * n + t_j) * n + t_k
    assert np.all(np.diff(key) > 0)                                                      # sorted by (row, j, k), no repeat
    # the rule itself: a row of L entries has sum_{s <= reach} (L - s) terms
    lens = np.diff(qp.rowptr).astype(np.int64)
    s = np.arange(1, c.reach + 1)
    assert np.array_equal(np.bincount(d.t_row, minlength=m), np.maximum(lens[:, None] - s[None, :], 0).sum(axis=1))
    a = dict(zip(pattern.tolist(), qp.vals.tolist()))
    some = np.random.default_rng(0).choice(d.nterms, min(d.nterms, 2000), replace=False)
    ratio = np.array([abs(d.t_w[t]) / np.sqrt(abs(a[t_row[t] * n + t_j[t]] * a[t_row[t] * n + t_k[t]])) for t in some])
    lo, hi = K.CURV / np.sqrt(c.reach) * 0.5, K.CURV / np.sqrt(c.reach) * 1.5
    assert ratio.min() >= lo * (1 - 1e-12) and ratio.max() <= hi * (1 + 1e-12) and (d.t_w < 0).any() and (d.t_w > 0).any()
    again = K.with_reach(qp, K.CURV, c.reach, K.SEED)
    assert np.array_equal(again.t_w, d.t_w) and np.array_equal(again.b, d.b) and np.array_equal(again.t_k, d.t_k)
    # the numpy restatement of the device's list builder takes them (every term, or the terms of every step-th row, step odd
    # so that every row length of a repeated pattern of lengths is met)
    step = (-(-d.nterms // LIST_TERMS)) | 1
    sel = np.flatnonzero(d.t_row % step == 0) if d.nterms > LIST_TERMS else np.arange(d.nterms)
    t_perm = np.lexsort((rows, qp.colind))
    lists = build_lists(n, m, qp.rowptr, qp.colind, np.arange(m), t_perm, d.t_row[sel], d.t_j[sel], d.t_k[sel], d.t_w[sel])
    assert sum(len(p) for p in lists["partners"]) == 2 * sel.size == sum(len(p) for p in lists["contrib"])
    if sel.size == d.nterms:
        assert lists["sci"].size == c.snz and int(np.diff(lists["srp"]).max()) == c.longest


@pytest.mark.parametrize("name", K.NAMES)
def test_the_couplings_matter_and_the_jacobian_is_well_posed(name):
    """at delta = sqrt(eps), (rho, eta) = (1, 0.5): dropping the terms (tests/sepquad_ref.py on the same a, h, b) moves the
    yardstick's gx and c by more than 1e-3 relative -- tests/test_band_coupled_nlp_cpu.py's threshold --, so the 1e-9 bar of the
    GPU test tells the models apart; sigma_min(J(x)) > 0.05 by dense SVD, tests/test_lane_groups_cpu.py's threshold."""
    d = K.data(name)
    qp = d.qp
    e = K.expected(name, SE)[(1.0, 0.5)]
    sep = SepQuadRef(cc.without_terms(d), K.SIGMA, 1.0, SE, 0.5, qp.xhat)
    e0 = sep.objgrad(qp.x)
    moved = {"gx": _rel(e0["gx"], e["gx"]), "c": _rel(e0["c"], e["c"]), "Hv2": _rel(sep.hprod(qp.x, K.v_of(qp), 2), e["Hv2"])}
    s = np.linalg.svd(nlpmodels.CoupledQuadConModel(d)._J(qp.x).toarray(), compute_uv=False)
    print(f"\n{name}: moved " + " ".join(f"{k}={v:.1e}" for k, v in moved.items())
          + f" |Hv1-Hv2|={_rel(e['Hv1'], e['Hv2']):.1e} sigma_min(J(x))={s[-1]:.3e} cond={s[0] / s[-1]:.1f}")
    for k, v in moved.items():
        assert v > 1e-3, (k, v)
    assert _rel(e["Hv1"], e["Hv2"]) > 1e-6
    assert s[-1] > 0.05


@pytest.mark.parametrize("name", K.NAMES)
def test_the_yardstick_solves_its_own_system(name):
    """as test_the_nonlinear_yardstick_solves_its_own_system of tests/test_lane_groups_cpu.py: with K = [I J'; J -delta I] and
    J = J(x), terms included, K [gs; ys] = [g; sigma c]; the residual of each block row relative to its largest term must be
    <= 1e-12, three decades under the device's 1e-9 bar."""
    d = K.data(name)
    qp = d.qp
    x = qp.x
    J = nlpmodels.CoupledQuadConModel(d)._J(x)
    g = qp.qdiag * x + qp.d
    for delta in K.deltas(name):
        e = K.expected(name, delta)[K.pairs(name)[0]]           # (ys, gs, c depend on sigma and delta alone)
        top = e["gs"] + J.T @ e["ys"] - g
        bottom = J @ e["gs"] - delta * e["ys"] - K.SIGMA * e["c"]
        scale_t = max(np.abs(e["gs"]).max(), np.abs(J.T @ e["ys"]).max(), np.abs(g).max())
        scale_b = max(np.abs(J @ e["gs"]).max(), K.SIGMA * np.abs(e["c"]).max())
        rt, rb = np.abs(top).max() / scale_t, np.abs(bottom).max() / scale_b
        print(f"\n{name} delta={delta:.1e}: KKT residual {rt:.2e} (n rows) {rb:.2e} (m rows)")
        assert rt <= 1e-12 and rb <= 1e-12
        assert _rel(e["c"], nlpmodels.CoupledQuadConModel(d).cons(x)) < 1e-13
