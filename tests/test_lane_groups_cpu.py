"""The case table of tests/lane_group_cases.py as far as it can be checked without a GPU: the literals of every case (sizes,
nnz, the three lane groups, the ragged-tile facts the case is there for), what the symbolic phase makes of it, the yardsticks
against themselves, and that the table reaches every lane-group width at every WITH_LANE_GROUP site of the band unit."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import nlpmodels, problems, qdsolver  # noqa: E402
import lane_group_cases as L  # noqa: E402
from sepquad_ref import SepQuadRef  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fletcherpenaltysolver.jl_amd", "csrc")
SE = L.SE

# case: (n % rows of an A' tile, m % rows of an A tile, mpad % rows of an A tile, A' tiles, A tiles over mpad); a tile has
# 256 // LG rows.  mpad is a multiple of 128, so the padded A side is ragged nowhere; m (k_bn_cons, jac_mul) and n are.
TILES = {
    "wide-rows": (0, 0, 0, 48, 32),          # m = 96 < 128: ONE partial block of the factor, 24 of the 32 A tiles hold rows
    "m-near-n": (4, 0, 0, 138, 128),
    "both-64": (0, 0, 0, 150, 128),          # n and mpad = 512 multiples of RPB = 4, m = 500 below mpad: three all-padding tiles
    "lgT-16": (8, 4, 0, 63, 64),
    "lgT-8": (24, 2, 0, 44, 48),
    "thin": (132, 188, 0, 4, 3),             # RPB = 256 on both sides
    "lg2": (132, 44, 0, 4, 3),
    "ragged": (4, 0, 0, 163, 128),
    "stride": (0, 0, 0, 2250, 2080),         # both above the cap of 2048: a second trip of every grid-stride loop
    "lg4-2": (48, 24, 0, 10, 10),
    "lg8-4": (16, 28, 0, 57, 48),
    "lg16-2": (80, 10, 0, 16, 16),
    "both-64-shuffled": (0, 0, 0, 150, 128),
    "ragged-shuffled": (4, 0, 0, 163, 128),
}


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def test_one_length_for_every_row_is_pde_control_like():
    a = L.ragged_band(4000, 400, (16,), 512, 21)
    b = problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21)
    for name in ("rowptr", "colind", "vals", "qdiag", "d", "b", "x", "xhat"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_the_restated_rule_is_the_one_of_the_header():
    """lane_group of csrc/fpsq_lanegroup.h, statement by statement, and the seven widths WITH_LANE_GROUP dispatches"""
    src = open(os.path.join(CSRC, "fpsq_lanegroup.h")).read()
    assert "const int64_t mean = rows > 0 ? nnz / rows : 1;" in src
    assert "while (lg < 64 && 2 * lg <= mean) lg *= 2;" in src
    assert tuple(int(w) for w in re.findall(r"constexpr int LG = (\d+);", src)) == L.WIDTHS
    assert [L.lane_group(k, 1) for k in (0, 1, 2, 3, 4, 63, 64, 127, 128, 10**6)] == [1, 1, 2, 2, 4, 32, 64, 64, 64, 64]
    band = open(os.path.join(CSRC, "fpsq_band.hip")).read()
    assert f"constexpr int kBqMaxGrid = {L.MAX_GRID};" in band
    # every per-entry launch of the nonlinear model (k_bn_vals, k_bcn_vals, k_bcn_assemble, the gathers of the create and of an
    # objgrad) takes its grid from ONE helper with that cap: no other launch of the file spells a grid of 256-entry blocks
    nlp = open(os.path.join(CSRC, "fpsq_band_nlp.hip.h")).read()
    assert nlp.count(f"dim3 flat_grid(int64_t len) {{ return dim3((unsigned)std::max<int64_t>(std::min<int64_t>((len + 255) / 256, "
                     f"{L.MAX_GRID_FLAT}), 1)); }}") == 1
    assert nlp.count("+ 255) / 256") == 1
    for kernel in ("k_bn_vals", "k_bcn_vals", "k_bcn_assemble", "k_gather_d"):
        launches = re.findall(rf"hipLaunchKernelGGL\({kernel}, (\w+)", nlp)
        assert launches and set(launches) <= {"flat_grid", "gz", "gt"}, kernel
    assert "const dim3 gz = flat_grid(b->nnz), gt = flat_grid(b->t_nnz);" in nlp


@pytest.mark.parametrize("name", L.NAMES)
def test_the_table_is_what_the_generator_and_the_rule_give(name):
    c, qp = L.CASES[name], L.qp(name)
    A = qp.scipy_csr()
    assert (qp.n, qp.m, qp.nnz) == (c.n, c.m, c.nnz)
    assert (L.lane_group(qp.nnz, qp.m), L.lane_group(qp.nnz, qp.n)) == (c.lgA, c.lgT)
    rows, cols = np.diff(A.indptr), np.bincount(A.indices, minlength=qp.n)
    assert (rows.min(), rows.max()) == c.rows
    assert (int((cols == 0).sum()), cols[cols > 0].min(), cols.max()) == c.cols
    rpa, rpt = 256 // c.lgA, 256 // c.lgT
    assert (c.n % rpt, c.m % rpa, c.mpad % rpa, L.tiles(c.n, c.lgT), L.tiles(c.mpad, c.lgA)) == TILES[name]
    assert np.abs(A @ qp.xhat - qp.b).max() < 1e-12
    if c.base is not None:   # the same rows in another order
        base = L.qp(c.base).scipy_csr()
        assert sorted(map(tuple, np.round(A.toarray(), 12))) == sorted(map(tuple, np.round(base.toarray(), 12)))
        assert not np.array_equal(A.indptr, base.indptr) or not np.array_equal(A.indices, base.indices)


def test_what_each_case_is_there_for():
    C = L.CASES
    # rows against the lane group: 2.5 LG; 1, 7, 13 (< LG), LG + 1, 2 LG, 2 LG + 1, 3 LG + 1, 6 LG + 8 under one LG; rows
    # shorter than LG at LG = 2 and 4
    assert C["wide-rows"].rows[0] * 2 == 5 * C["wide-rows"].lgA and C["wide-rows"].cols[1] < C["wide-rows"].lgT
    lg = C["ragged"].lgA
    assert sorted(C["ragged"].lens) == [1, 7, 13, lg + 1, 2 * lg, 2 * lg + 1, 3 * lg + 1, 6 * lg + 8]
    assert all(k % C["lgT-8"].lgA for k in C["lgT-8"].lens)
    assert C["lg2"].rows[0] < C["lg2"].lgA < C["lg2"].rows[1] and C["lg4-2"].rows[0] < C["lg4-2"].lgA < C["lg4-2"].rows[1]
    assert C["thin"].cols[0] == 146 and C["lg2"].cols[0] == 361            # columns that receive no product term
    # columns shorter than their lane group on the A' side: lanes that never enter the k < e loop while the shuffles run
    for name in ("wide-rows", "m-near-n", "both-64", "lgT-16", "lgT-8", "ragged", "stride", "lg4-2", "lg8-4", "lg16-2"):
        assert C[name].cols[1] < C[name].lgT, name
    # the three caps together, and no larger than it has to be
    s = C["stride"]
    assert L.tiles(s.n, s.lgT) > L.MAX_GRID and L.tiles(s.mpad, s.lgA) > L.MAX_GRID and L.tiles(s.m, s.lgA) > L.MAX_GRID
    assert s.nnz > L.MAX_GRID_FLAT * 256 and s.band["chains"] == 2
    assert all(L.tiles(max(c.n, c.mpad), min(c.lgA, c.lgT)) <= L.MAX_GRID for k, c in C.items() if k != "stride")
    assert C["wide-rows"].m < 128 and C["both-64"].m < C["both-64"].mpad == 512


def test_the_widths_the_table_reaches():
    """every width on the A side, on the A' side and on the Hessian's, within this table"""
    assert {c.lgA for c in L.CASES.values()} == set(L.WIDTHS)
    assert {c.lgT for c in L.CASES.values()} == set(L.WIDTHS)
    assert set(L.HESS_HALF_WIDTHS) == set(L.WIDTHS)
    for (name, hw), lgr in L.HESS_CASES.items():
        assert L.hessian_lanes(L.hess_qp(name, hw)) == lgr, (name, hw)
    for lgr, hw in L.HESS_HALF_WIDTHS.items():   # the smallest half-width that reaches it (just over LG / 2, as the rows at
        if hw > 1:                               # the edges and the empty rows of with_sparse_hessian pull the mean down)
            assert L.hessian_lanes(L.hess_qp(L.HESS_BASE, hw - 1)) < lgr
    assert L.qp(L.HESS_BASE).n == 1100 and 64 in L.HESS_HALF_WIDTHS    # 64 lanes are reached at n = 1100: no exception
    # the Hessian as a template flag of the A-side and A'-side kernels: every width on each side
    hess = [L.CASES[name] for name, _ in L.HESS_CASES]
    assert {c.lgA for c in hess} == set(L.WIDTHS) and {c.lgT for c in hess} == set(L.WIDTHS)
    # the widths under which the rows of a shuffled handle are read through rperm / vperm / t_perm
    assert {(c.lgA, c.lgT) for c in L.CASES.values() if c.band["reordered"]} == {(64, 64), (32, 32)}


@pytest.mark.parametrize("name", L.NAMES)
def test_the_symbolic_phase_takes_every_case(name):
    info = qdsolver.band_analysis(nlpmodels.EqQPModel(L.qp(name)))
    assert info is not None, "the analysis refuses the shape: change its window"
    print(f"\n{name}: " + " ".join(f"{k}={info[k]}" for k in ("chains", "nblocks", "bandwidth_blocks", "reordered")))
    assert {k: info[k] for k in L.CASES[name].band} == L.CASES[name].band
    assert info["border_rows"] == 0 and info["border_cols"] == 0


def test_the_site_table_names_every_dispatch_of_the_band_unit():
    """every kernel launched under WITH_LANE_GROUP in fpsq_band.hip and fpsq_band_nlp.hip.h has a row in the docstring table:
    EVERY kernel named inside the balanced parentheses of an invocation (a dispatch may launch one kernel or another: the
    function forms sit in the `else` branches of the separable model's dispatches), not the first alone.  Where one invocation
    names the same kernel twice, the second instantiation needs a row that spells its template arguments."""
    sites, first_only = [], []
    for f in ("fpsq_band.hip", "fpsq_band_nlp.hip.h"):
        src = open(os.path.join(CSRC, f)).read()
        first_only += re.findall(r"WITH_LANE_GROUP\((?:qp->|lin\.)?(\w+),.*?\(?(k_\w+)<", src, flags=re.S)
        for inv in re.finditer(r"WITH_LANE_GROUP\(", src):
            end, depth = inv.end(), 1
            while depth:
                depth += {"(": 1, ")": -1}.get(src[end], 0)
                end += 1
            body = src[inv.end():end - 1]
            lg = re.match(r"\s*(?:qp->|lin\.)?(\w+),", body).group(1)
            named = re.findall(r"\b(k_\w+)\s*(<[^>]*>|(?=\)))", body)
            assert named, body
            for i, (kernel, targs) in enumerate(named):
                sites.append((lg, kernel, re.sub(r"\s+", " ", targs) if kernel in [k for k, _ in named[:i]] else None))
    assert len(first_only) == 30 and set(first_only) <= {(lg, kernel) for lg, kernel, _ in sites}   # what the first name gave
    assert len(sites) == 33   # (18 in fpsq_band.hip, 15 in fpsq_band_nlp.hip.h: 12 dispatches, three with a function form)
    assert {lg for lg, _, _ in sites} == {"lgA", "lgT", "lgR", "lg"}
    for _, kernel, targs in sites:
        assert re.search(rf"^\s+{kernel}\b", L.__doc__, flags=re.M), kernel
        if targs is not None:
            assert re.search(rf"^\s+{re.escape(kernel + targs)}\s", L.__doc__, flags=re.M), kernel + targs
    assert {(k, t) for _, k, t in sites if k.endswith("_fn") or t} == {("k_bn_cons_fn", None), ("k_bn_tvals_fn", None),
                                                                         ("k_bn_prologue", "<LG, false, true>")}


def test_the_widths_the_coupled_cases_reach():
    """what the site table says the model with coupling terms (the CP forms and the k_bcn_* row kernels) runs at: recomputed
    from tests/coupled_cases.py, every case of the GPU suite and its `stride`"""
    import coupled_cases as cc

    reach = {}
    for name in list(cc.CASES) + ["stride"]:
        d = cc.data(name)
        reach[name] = (L.lane_group(d.qp.nnz, d.qp.m), L.lane_group(d.qp.nnz, d.qp.n), L.lane_group(cc.s_pattern(d)[1], d.qp.n))
    print("\n" + "  ".join(f"{k}: {v}" for k, v in reach.items()))
    lga, lgt, lgr = ({v[i] for v in reach.values()} for i in range(3))
    assert (lga, lgt, lgr) == ({2, 4, 16, 32}, {1, 2, 32}, {1, 8})
    assert reach["stride"] == (2, 1, 1)
    doc = L.__doc__
    assert "lgA 2, 4, 16, 32; lgT 1, 2, 32; lgR 1, 8" in doc and "STRIDE at 2 / 1 / 1" in doc


@pytest.mark.parametrize("name", L.NAMES)
def test_the_nonlinear_yardstick_solves_its_own_system(name):
    """SepQuadRef at x = qp.x: with K = [I J'; J -delta I] and J = J(x), K [gs; ys] = [g; sigma c].  The residual of that
    system, relative to the largest term of each block row, must be <= 1e-12: three decades under the device's 1e-9 bar."""
    qp = L.qp(name)
    x = qp.x
    J = nlpmodels.SepQuadConModel(L.nlp_data(name))._J(x)
    if qp.m <= 1500:
        s = np.linalg.svd(J.toarray(), compute_uv=False)
        print(f"\n{name}: sigma_min(J(x)) = {s[-1]:.3e}, cond(J(x)) = {s[0] / s[-1]:.2f}")
        assert s[-1] > 0.05
    for delta in (SE,) if name == "stride" else (0.0, SE):
        ref = L.exact_nonlinear(name, delta)
        e = ref.objgrad(x)
        g = qp.qdiag * x + qp.d
        top = e["gs"] + J.T @ e["ys"] - g
        bottom = J @ e["gs"] - delta * e["ys"] - L.SIGMA * e["c"]
        scale_t = max(np.abs(e["gs"]).max(), np.abs(J.T @ e["ys"]).max(), np.abs(g).max())
        scale_b = max(np.abs(J @ e["gs"]).max(), L.SIGMA * np.abs(e["c"]).max())
        rt, rb = np.abs(top).max() / scale_t, np.abs(bottom).max() / scale_b
        print(f"{name} delta={delta:.1e}: KKT residual {rt:.2e} (n rows) {rb:.2e} (m rows)")
        assert rt <= 1e-12 and rb <= 1e-12


def test_the_kept_factors_change_nothing():
    """the yardsticks with their factor kept against the ones that refactorise per call: the same definitions"""
    from oracle import oracle

    for name, bar in (("lg8-4", 1e-13), ("thin", 1e-12)):   # n + m above / below the oracle's switch to a dense solve
        qp = L.qp(name)
        v = np.random.default_rng(0).standard_normal(qp.n)
        for delta in (0.0, SE):
            ref = L.exact_linear(name, delta)
            a, b = ref.objgrad(qp.x, L.SIGMA, 1.0, 0.5, qp.xhat), oracle.exact_qp_objgrad(qp, qp.x, L.SIGMA, 1.0, delta, 0.5,
                                                                                         qp.xhat)
            assert all(_rel(a[k], b[k]) <= bar for k in ("gx", "ys", "gs")) and abs(a["fx"] - b["fx"]) <= bar * abs(b["fx"])
            assert _rel(ref.hprod(v, L.SIGMA, 1.0, 0.5), oracle.exact_qp_hprod(qp, v, L.SIGMA, 1.0, delta, 0.5)) <= bar
    name = "lgT-8"
    qp, data = L.qp(name), L.nlp_data(name)
    v = np.random.default_rng(0).standard_normal(qp.n)
    kept, plain = L.exact_nonlinear(name, SE), SepQuadRef(data, L.SIGMA, 1.0, SE, 0.5, qp.xhat)
    kept.pen.rho, kept.pen.eta = 1.0, 0.5
    a, b = kept.objgrad(qp.x), plain.objgrad(qp.x)
    assert all(_rel(a[k], b[k]) <= 1e-12 for k in ("gx", "ys", "gs", "c")) and abs(a["fx"] - b["fx"]) <= 1e-12 * abs(b["fx"])
    for approx in (2, 1):
        assert _rel(kept.hprod(qp.x, v, approx), plain.hprod(qp.x, v, approx)) <= 1e-12
    kept.pen.rho, kept.pen.eta = 0.0, 0.0
