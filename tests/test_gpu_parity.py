"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
 (a) the reference's own known-answer tests (tests/golden/),
 (b) the C restatement of the reference's iterative back-end (oracle/fps_oracle.c), iteration for iteration,
 (c) the exact KKT solve.
Tolerances are written at each assertion; everything is fp64."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import fps_amd  # noqa: F401
from fps_amd import _lib, nlpmodels, problems
from fps_amd.device_qp import DeviceEqQP
from fps_amd.penalty_nlp import FletcherPenaltyNLP
from fps_amd.qdsolver import HIPQDSolver

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_known_answers.json")))["cases"]
SE = np.sqrt(np.finfo(float).eps)
TIGHT = dict(ls_atol=1e-15, ls_rtol=1e-15, ls_axtol=1e-15, ls_btol=1e-15, ls_etol=1e-15,
             ln_atol=1e-15, ln_rtol=1e-15, ln_btol=1e-15, ln_conlim=0.0)


from abi_handle import _Handle, _rel  # noqa: E402  (tests/abi_handle.py: shared with tests/test_gpu_lane_structures.py)


# ---------------------------------------------------------------------------------------------- SpMV

def _spmv_cases():
    rng = np.random.default_rng(0)
    cases = {}
    cases["random"] = sp.random(300, 1000, density=0.02, random_state=rng, format="csr")
    A = sp.random(64, 5000, density=0.3, random_state=rng, format="lil")
    A[3, :] = rng.standard_normal(5000)  # one row longer than the 2048-nnz LDS stage
    A[10, :] = 0  # and empty rows
    A[11, :] = 0
    cases["long_and_empty_rows"] = A.tocsr()
    cases["single_row"] = sp.csr_matrix(np.ones((1, 10)))
    cases["ragged"] = sp.vstack([sp.random(1, 3000, density=d, random_state=rng, format="csr")
                                 for d in (0.0, 0.001, 0.9, 0.0, 0.3, 0.001, 0.7, 0.0)]).tocsr()
    cases["tall"] = sp.random(5000, 40, density=0.1, random_state=rng, format="csr")
    B = sp.random(3000, 50, density=0.05, random_state=rng, format="lil")
    B[:, 7] = rng.standard_normal((3000, 1))  # a dense column: A' gets a row longer than the LDS stage (unpadded A')
    cases["dense_column"] = B.tocsr()
    return cases


@pytest.mark.parametrize("fmt", [0, 1])  # 0: RGCS / padded / 16-bit-column layouts where representable, 1: plain CSR
@pytest.mark.parametrize("name", list(_spmv_cases()))
def test_spmv_matches_oracle(oracle, name, fmt):
    A = sp.csr_matrix(_spmv_cases()[name])
    A.sort_indices()
    m, n = A.shape
    rng = np.random.default_rng(1)
    H = _Handle(A, jac_format=fmt)
    x, u = rng.standard_normal(n), rng.standard_normal(m)
    y0, z0 = rng.standard_normal(m), rng.standard_normal(n)
    want = 1.5 * oracle.spmv(m, n, A.indptr, A.indices, A.data, x) - 0.5 * y0
    got = H.jac_mul(0, 1.5, x, -0.5, y0)
    # different summation order only: 1e-13 relative to the row's |a|.|x| mass
    scale = np.abs(A) @ np.abs(x) + np.abs(y0) + 1e-300
    assert np.max(np.abs(got - want) / scale) < 1e-13
    want = -2.0 * oracle.spmv(m, n, A.indptr, A.indices, A.data, u, transposed=True)
    got = H.jac_mul(1, -2.0, u, 0.0, np.full(n, np.nan))  # beta = 0 must not read y
    scale = np.abs(A).T @ np.abs(u) + 1e-300
    assert np.all(np.isfinite(got)) and np.max(np.abs(got - want) / scale) < 1e-13
    got2 = H.jac_mul(1, -2.0, u, 0.0, z0)
    assert np.array_equal(got, got2), "SpMV must be bitwise reproducible"
    H.close()


@pytest.mark.parametrize("seed", range(12))
def test_spmv_random_structures_layouts_agree(seed):
    """Randomised structures (row lengths from 0 to several LDS stages, banded and scattered columns, sizes that are
    not multiples of any tile): the tuned layouts (RGCS groups, padded blocks, 16-bit columns) and plain CSR must give
    the same products to rounding, and a two-system solve the same iteration counts."""
    rng = np.random.default_rng(1000 + seed)
    m = int(rng.integers(1, 700))
    n = int(rng.integers(max(2, m // 4), 6000))
    kind = seed % 4
    rows, cols = [], []
    for i in range(m):
        if kind == 0:    # short scattered rows, many empty
            k = int(rng.integers(0, 6))
            c = rng.choice(n, size=min(k, n), replace=False)
        elif kind == 1:  # banded, ~100 per row (the headline shape in small)
            w = min(n, 900)
            lo = int(rng.integers(0, n - w + 1))
            c = lo + rng.choice(w, size=min(100, w), replace=False)
        elif kind == 2:  # wildly different row lengths including rows longer than one LDS stage
            k = int(rng.choice([0, 1, 3, 50, 400, 2500, 5000]))
            c = rng.choice(n, size=min(k, n), replace=False)
        else:            # dense-ish narrow matrix: long rows of A' (dense columns)
            c = rng.choice(n, size=max(1, n // 3), replace=False)
        rows += [i] * len(c)
        cols += list(c)
    A = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(m, n))
    A.sum_duplicates()
    A.sort_indices()
    if A.nnz == 0:
        A = sp.csr_matrix(([1.0], ([0], [0])), shape=(m, n))
    x, u = rng.standard_normal(n), rng.standard_normal(m)
    y0, z0 = rng.standard_normal(m), rng.standard_normal(n)
    H0, H1 = _Handle(A, jac_format=0), _Handle(A, jac_format=1)
    for trans, vec, add in ((0, x, y0), (1, u, z0)):
        a = H0.jac_mul(trans, 0.75, vec, -1.25, add)
        b = H1.jac_mul(trans, 0.75, vec, -1.25, add)
        ref = 0.75 * ((A.T if trans else A) @ vec) - 1.25 * add
        scale = np.abs(A.T if trans else A) @ np.abs(vec) + np.abs(add) + 1e-300
        assert np.max(np.abs(a - ref) / scale) < 1e-13 and np.max(np.abs(b - ref) / scale) < 1e-13
    if m <= n:  # a full-row-rank-ish system: both layouts run the same recurrences
        g, c = rng.standard_normal(n), rng.standard_normal(m)
        r0 = H0.solve_two_mixed(g, c)
        it0 = (H0.st[0].niter, H0.st[1].niter)
        r1 = H1.solve_two_mixed(g, c)
        # (ill-conditioned draws run thousands of iterations: rounding differences may shift the stop by a few)
        for k in range(2):
            assert abs(H1.st[k].niter - it0[k]) <= max(1, it0[k] // 50)
        if r0[4] == 0 and r1[4] == 0 and (H1.st[0].niter, H1.st[1].niter) == it0:
            for a, b in zip(r0[:4], r1[:4]):
                assert _rel(a, b) < 1e-7
    H0.close()
    H1.close()


@pytest.mark.parametrize("fmt", [0, 1])  # 1: the CSR fallback serves the A product (its array is then a destination too)
@pytest.mark.parametrize("how", ["csr", "coo", "coo-dup"])
def test_one_pass_jacobian_refresh_is_bitwise_the_three_pass_one(monkeypatch, how, fmt):
    """fpsq_set_jacobian_values = `jac_coord!` at a new x (src/solve_linear_system.jl:118-122, :223-228).  One gather launch
    (k_refresh: permutations composed down to the caller's array at structure time) writes the row-group copy of A, the
    column-sorted blocks of A' and -- only where a product reads it -- the CSR array; device-resident values are read in
    place and ordered on the registered stream.  Pure copies (duplicates summed in the same fixed order): products and
    solves must be BITWISE those of a handle that refreshes with the three grid-stride passes of rounds 1-3
    (FPSQ_JAC_REFRESH=3), for CSR input, COO input, COO input with duplicates, host and device values, and after a SECOND
    refresh with other values (nothing stale)."""
    import torch

    qp = _small_pde(seed=31, n=30000, m=3000)
    rng = np.random.default_rng(8)
    rows = np.repeat(np.arange(qp.m), np.diff(qp.rowptr)).astype(np.int64)
    cols = qp.colind.astype(np.int64)
    nnz = qp.nnz
    if how == "csr":
        struct = None
        values = [qp.vals.copy(), qp.vals * (1.0 + 0.1 * rng.standard_normal(nnz))]
    else:
        perm = rng.permutation(nnz)  # the model's own (unsorted) triplet order
        r, c = rows[perm], cols[perm]
        values = [qp.vals[perm].copy(), (qp.vals * (1.0 + 0.1 * rng.standard_normal(nnz)))[perm]]
        if how == "coo-dup":  # a tenth of the entries split into two triplets
            k = rng.choice(nnz, nnz // 10, replace=False)
            r, c = np.concatenate([r, r[k]]), np.concatenate([c, c[k]])
            values = [np.concatenate([v * np.where(np.isin(np.arange(nnz), k), 0.25, 1.0), 0.75 * v[k]]) for v in values]
        struct = (r + 1, c + 1)  # (1-based, as NLPModels hands them over)
    lib = _lib.load()
    x, u = rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    g, cc = rng.standard_normal(qp.n), rng.standard_normal(qp.m)

    def run(where):
        o = _lib.Options()
        lib.fpsq_default_options(qp.n, qp.m, C.byref(o))
        o.jac_format = fmt
        h = C.c_void_p()
        assert lib.fpsq_create(C.byref(h), qp.n, qp.m, C.byref(o)) == 0
        if struct is None:
            rp, ci = qp.rowptr.astype(np.int32), qp.colind.astype(np.int32)
            assert lib.fpsq_set_jacobian_structure_csr(h, rp.ctypes.data, ci.ctypes.data) == 0
        else:
            rr, cq = np.ascontiguousarray(struct[0]), np.ascontiguousarray(struct[1])
            assert lib.fpsq_set_jacobian_structure_coo(h, rr.size, rr.ctypes.data, cq.ctypes.data, 1) == 0
        out = []
        st = (_lib.Stats * 2)()
        keep = []
        for v in values:
            if where == "device":
                t = torch.from_numpy(np.ascontiguousarray(v)).cuda()
                keep.append(t)
                assert lib.fpsq_set_input_stream(h, 1, int(torch.cuda.current_stream().cuda_stream)) == 0
                assert lib.fpsq_set_jacobian_values(h, t.data_ptr()) == 0, lib.fpsq_last_error(h)
                t.mul_(0.0)  # queued on the registered stream BEHIND the gathers that read t: must not reach them
            else:
                vv = np.ascontiguousarray(v)
                assert lib.fpsq_set_jacobian_values(h, vv.ctypes.data) == 0, lib.fpsq_last_error(h)
            y, z = np.zeros(qp.m), np.zeros(qp.n)
            assert lib.fpsq_jac_mul(h, 0, 1.0, x.ctypes.data, 0.0, y.ctypes.data) == 0
            assert lib.fpsq_jac_mul(h, 1, 1.0, u.ctypes.data, 0.0, z.ctypes.data) == 0
            o4 = [np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)]
            assert lib.fpsq_solve_two_mixed(h, g.ctypes.data, cc.ctypes.data, *[a.ctypes.data for a in o4], st) >= 0
            out += [y, z, *o4, np.array([st[0].niter, st[1].niter], dtype=float)]
        lib.fpsq_destroy(h)
        return out

    monkeypatch.setenv("FPSQ_JAC_REFRESH", "3")
    want = run("host")
    monkeypatch.setenv("FPSQ_JAC_REFRESH", "1")
    A0 = sp.csr_matrix((qp.vals, qp.colind, qp.rowptr), shape=(qp.m, qp.n))
    assert _rel(want[0], A0 @ x) < 1e-13 and _rel(want[1], A0.T @ u) < 1e-13  # (the first set of values IS the model's Jacobian)
    for where in ("host", "device"):
        got = run(where)
        for i, (a_, b_) in enumerate(zip(got, want)):
            assert np.array_equal(a_, b_), (where, i)


def test_coo_structure_with_duplicates_matches_sparse_sum():
    """jac_structure! may repeat (i, j); SparseArrays.sparse sums duplicates (src/solve_linear_system.jl:233)."""
    rng = np.random.default_rng(3)
    m, n, k = 50, 200, 900
    rows = rng.integers(1, m + 1, k).astype(np.int64)
    cols = rng.integers(1, n + 1, k).astype(np.int64)
    vals = rng.standard_normal(k)
    A = sp.coo_matrix((vals, (rows - 1, cols - 1)), shape=(m, n)).tocsr()
    assert A.nnz < k  # duplicates present
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.fpsq_create(C.byref(h), n, m, None) == 0
    assert lib.fpsq_set_jacobian_structure_coo(h, k, rows.ctypes.data, cols.ctypes.data, 1) == 0
    assert lib.fpsq_set_jacobian_values(h, vals.ctypes.data) == 0
    x = rng.standard_normal(n)
    y = np.zeros(m)
    assert lib.fpsq_jac_mul(h, 0, 1.0, x.ctypes.data, 0.0, y.ctypes.data) == 0
    np.testing.assert_allclose(y, A @ x, rtol=0, atol=1e-12 * np.linalg.norm(x))
    u = rng.standard_normal(m)
    z = np.zeros(n)
    assert lib.fpsq_jac_mul(h, 1, 1.0, u.ctypes.data, 0.0, z.ctypes.data) == 0
    np.testing.assert_allclose(z, A.T @ u, rtol=0, atol=1e-12 * np.linalg.norm(u))
    lib.fpsq_destroy(h)


# ---------------------------------------------------------------------------------------------- golden vectors

_MODELS = {"sumsq": lambda: nlpmodels.SumSquares(10), "rosenbrock_circle": nlpmodels.RosenbrockCircle}


@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_reference_known_answers_through_hip_backend(case):
    """The reference's own assertions (test/unit-test.jl, cited in the fixture) with the MI355X back-end plugged
    into the QDSolver seam.  Krylov tolerances are tightened so the LDLt-level atol of the reference test applies
    (x4 slack for the iterative path)."""
    nlp = _MODELS[case["model"]]()
    qds = HIPQDSolver(nlp, 0.0, **TIGHT)
    fp = FletcherPenaltyNLP(nlp, case["sigma"], case["rho"], case["delta"], 1, qds=qds)
    x = np.array(case["x"])
    got = dict(obj=fp.obj(x), fx=fp.fx, gx=fp.gx.copy(), ys=fp.ys.copy(), cx=fp.cx.copy())
    if "grad" in case["expect"]:
        got["grad"] = fp.grad(x)
    fobj, g2 = fp.objgrad(x)
    assert fobj == pytest.approx(got["obj"], abs=1e-14)  # unit-test.jl:128-129
    for key, want in case["expect"].items():
        atol = max(case["atol"][key], 1e-15) * 4
        np.testing.assert_allclose(got[key], want, rtol=0, atol=atol, err_msg=f"{case['name']}:{key}")
    assert qds.stats[0].solved and qds.stats[1].solved
    if "hprod" in case:  # unit-test.jl:190-191, 201-202: both Hessian approximations share this closed form here
        for approx in (2, 1):
            fp2 = FletcherPenaltyNLP(nlp, case["sigma"], case["rho"], case["delta"], approx, qds=qds)
            hv = fp2.hprod(x, np.array(case["hprod"]["v"]))
            np.testing.assert_allclose(hv, case["hprod"]["expect"], rtol=0, atol=case["hprod"]["atol"] * 4,
                                       err_msg=f"{case['name']}:hprod Val({approx})")
    qds.close()


def test_hprod_both_backends_agree_on_nonlinear_constraints():
    """hprod! Val(1)/Val(2) (model-Fletcherpenaltynlp.jl:521-634) on Rosenbrock + circle (nonlinear constraint, so
    ghjvprod and solve_two_extras are exercised): the iterative and the direct MI355X back-ends agree."""
    from fps_amd.qdsolver import HIPDirectQDSolver

    nlp = nlpmodels.RosenbrockCircle()
    x = np.array([0.7, -0.4])
    v = np.array([0.3, 1.1])
    out = {}
    tight = {**TIGHT, "ne_atol": 1e-15, "ne_rtol": 1e-15, "ne_etol": 1e-15}
    for approx in (1, 2):
        it = FletcherPenaltyNLP(nlp, 0.5, 0.1, 0.25, approx, qds=HIPQDSolver(nlp, 0.0, **tight))
        out[("it", approx)] = it.hprod(x, v)
        it.qdsolver.close()
    d2 = FletcherPenaltyNLP(nlp, 0.5, 0.1, 0.25, 2, qds=HIPDirectQDSolver(nlp, 0.0))
    np.testing.assert_allclose(out[("it", 2)], d2.hprod(x, v), rtol=1e-10)
    d2.qdsolver.close()
    assert np.all(np.isfinite(out[("it", 1)])) and not np.allclose(out[("it", 1)], out[("it", 2)])


def test_hs6_plumbing_kkt_3x3(oracle):
    """BASELINE configs[0]: HS6 at x0; K is 3x3; the two solves against the exact KKT solution."""
    nlp = nlpmodels.HS6()
    qds = HIPQDSolver(nlp, 0.0, **TIGHT)
    fp = FletcherPenaltyNLP(nlp, 1e3, 1.0, 0.0, 2, qds=qds)
    x0 = nlp.meta.x0
    fp.obj(x0)
    A = sp.csr_matrix(np.array([[-20 * x0[0], 10.0]]))
    e = oracle.exact_two_mixed(A, 0.0, nlp.grad(x0), nlp.cons(x0))
    np.testing.assert_allclose(fp.ys, e[1] + 1e3 * e[3], rtol=1e-12)
    np.testing.assert_allclose(fp.gs, e[0] + 1e3 * e[2], rtol=0, atol=1e-10)
    qds.close()


# ---------------------------------------------------------------------------------------------- Krylov parity

def _small_pde(seed=7, n=4000, m=400):
    return problems.pde_control_like(n=n, m=m, per_row=20, window=512, seed=seed)


@pytest.mark.parametrize("fmt", [0, 1])  # every storage layout of the products must give the same recurrences
@pytest.mark.parametrize("delta", [0.0, SE, 0.25])
@pytest.mark.parametrize("fuse", [0, 1])
def test_solve_two_mixed_iteration_parity_with_c_restatement(oracle, delta, fuse, fmt):
    """Default reference tolerances: same iteration counts / statuses as the CPU restatement, vectors equal to
    1e-9 (relative inf-norm: only the summation order differs), and within 1e-6 of the exact solve."""
    qp = _small_pde()
    A = qp.scipy_csr()
    g = qp.qdiag * qp.x + qp.d
    c = A @ qp.x - qp.b
    H = _Handle(A, delta=delta, fuse_two_rhs=fuse, jac_format=fmt)
    p1, q1, p2, q2, rc = H.solve_two_mixed(g, c)
    o = oracle.solve_two_mixed(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, g, c)
    assert rc == o[5]
    for k in range(2):
        assert H.st[k].niter == o[4][k].niter and H.st[k].status == o[4][k].status
        assert H.st[k].solved == o[4][k].solved and H.st[k].inconsistent == o[4][k].inconsistent
        assert H.st[k].rnorm == pytest.approx(o[4][k].rnorm, rel=1e-6, abs=1e-300)
    e = oracle.exact_two_mixed(A, delta, g, c)
    for got, want_c, want_e in zip((p1, q1, p2, q2), o[:4], e):
        assert _rel(got, want_c) < 1e-9
        assert _rel(got, want_e) < 1e-6
    H.close()


from structures import ALL_KINDS, ORDER_SENSITIVE, WELL_CONDITIONED, random_structure as _random_structure  # noqa: E402


def _awkward_case(kind, delta, fuse, **opts):
    rng = np.random.default_rng(12)
    A = _random_structure(kind, rng)
    m, n = A.shape
    H = _Handle(A, delta=delta, fuse_two_rhs=fuse, **opts)
    x, u = rng.standard_normal(n), rng.standard_normal(m)
    As = sp.csr_matrix(A)
    assert _rel(H.jac_mul(0, 1.0, x, 0.0, np.zeros(m)), As @ x) < 1e-13
    assert _rel(H.jac_mul(1, 1.0, u, 0.0, np.zeros(n)), As.T @ u) < 1e-13
    g, c = rng.standard_normal(n), rng.standard_normal(m)
    r1, r2 = rng.standard_normal(n), rng.standard_normal(n)
    csr = (A.indptr.astype(np.int64), A.indices.astype(np.int64), np.ascontiguousarray(A.data))
    return H, As, m, n, csr, g, c, r1, r2


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("delta", [SE, 0.25])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_recurrences_agree_iteration_for_iteration_before_rounding_grows(oracle, kind, delta, fuse):
    """THE layout test of the awkward structures (unpadded A' when a row is longer than an LDS stage, a long row of A in a
    row group of its own, row-order A' blocks when a block spans more than 8192 columns, empty row blocks, a Jacobian of one
    row, unsorted CSR rows, m close to n).  Both programs are cut at k = 1, 2, 3 iterations (ls_itmax = ln_itmax = k): same
    iteration counts and statuses, the residual estimates (rnorm, arnorm) and all four solution vectors of solve_two_mixed
    and solve_two_least_squares equal to 1e-12 at k <= 2 and 1e-9 at k = 3.  A mis-placed entry, a dropped tail of a long
    row or a wrong norm partial is an O(1) difference at k = 1; what rounding alone does is 1e-15 there and grows from it
    (profiles/r04_fixed_iteration_probe.txt: x1000 per iteration on the dense-row case -- 1e-11 at k = 3 -- which is why the
    FINAL counts of three structures are compared with a spread below, and these with none)."""
    rng = np.random.default_rng(12)
    A = _random_structure(kind, rng)
    m, n = A.shape
    rng.standard_normal(n), rng.standard_normal(m)
    g, c = rng.standard_normal(n), rng.standard_normal(m)
    r1, r2 = rng.standard_normal(n), rng.standard_normal(n)
    rp, ci, va = A.indptr.astype(np.int64), A.indices.astype(np.int64), np.ascontiguousarray(A.data)
    for k in (1, 2, 3):
        tol = 1e-12 if k <= 2 else 1e-9
        H = _Handle(A, delta=delta, fuse_two_rhs=fuse, ls_itmax=k, ln_itmax=k)
        opts = oracle.default_options(n, m, ls_itmax=k, ln_itmax=k)
        d1 = H.solve_two_mixed(g, c)
        s1 = [(H.st[i].niter, H.st[i].status, H.st[i].solved, H.st[i].rnorm, H.st[i].arnorm) for i in range(2)]
        o1 = oracle.solve_two_mixed(m, n, rp, ci, va, delta, g, c, opts=opts)
        d2 = H.solve_two_least_squares(r1, r2)
        s2 = [(H.st[i].niter, H.st[i].status, H.st[i].solved, H.st[i].rnorm, H.st[i].arnorm) for i in range(2)]
        o2 = oracle.solve_two_least_squares(m, n, rp, ci, va, delta, r1, r2, opts=opts)
        H.close()
        for d, st, o in ((d1, s1, o1), (d2, s2, o2)):
            assert d[4] == o[5], k
            for i in range(2):
                w = o[4][i]
                assert st[i][:3] == (w.niter, w.status, w.solved), (k, i)
                # (relative to the estimate, or to the O(1) scale of the right-hand sides where it has reached rounding level)
                assert abs(st[i][3] - w.rnorm) <= tol * max(abs(w.rnorm), 1.0), (k, i)
                assert abs(st[i][4] - w.arnorm) <= tol * max(abs(w.arnorm), 1.0), (k, i)
            for got, want in zip(d[:4], o[:4]):
                assert _rel(got, want) < tol, k


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("delta", [SE, 0.25])
@pytest.mark.parametrize("kind", WELL_CONDITIONED)
def test_awkward_jacobian_structures_match_the_c_restatement(oracle, kind, delta, fuse):
    """Run to the reference's tolerances (sqrt(eps)), the four structures whose stop does not depend on rounding:
    A v / A' u equal scipy's to rounding; solve_two_mixed and solve_two_least_squares through the C ABI follow the CPU
    restatement to the end -- EQUAL iteration counts, statuses and solved flags -- and, at delta = 0.25, land within 1e-3 of the exact
    KKT solve (reference tolerances sqrt(eps)).  The vectors: only the summation order differs between the two programs, and
    how much THAT moves a vector is measured, not assumed -- the restatement is run a second time with every row summed right
    to left (oracle.set_sum_order(2): the same arithmetic, re-associated); the device must agree with the restatement to 1e-9
    or to 20 x the distance between those two runs, whichever is larger (1e-9 on most vectors; after 100 iterations of the
    wide-window case, or where CRAIG stops on its conditioning limit, the two CPU runs themselves are 1e-7 ... 1e-5 apart)."""
    H, As, m, n, (rp, ci, va), g, c, r1, r2 = _awkward_case(kind, delta, fuse)
    p1, q1, p2, q2, rc = H.solve_two_mixed(g, c)
    o = oracle.solve_two_mixed(m, n, rp, ci, va, delta, g, c)
    try:
        oracle.set_sum_order(2)
        ob = oracle.solve_two_mixed(m, n, rp, ci, va, delta, g, c)
        ob2 = oracle.solve_two_least_squares(m, n, rp, ci, va, delta, r1, r2)
    finally:
        oracle.set_sum_order(0)
    assert rc == o[5]
    for k in range(2):
        assert (H.st[k].niter, H.st[k].status, H.st[k].solved) == (o[4][k].niter, o[4][k].status, o[4][k].solved), k
    exact = delta > 1e-3 and n + m <= 7000  # (at delta = sqrt(eps) CRAIG may stop on its conditioning limit, far from the solve)
    e = oracle.exact_two_mixed(As, delta, g, c) if exact else o[:4]
    for got, want, alt, ex in zip((p1, q1, p2, q2), o[:4], ob[:4], e):
        assert _rel(got, want) < max(1e-9, 20 * _rel(alt, want)) and _rel(got, ex) < 1e-3
    p1, q1, p2, q2, rc = H.solve_two_least_squares(r1, r2)
    o = oracle.solve_two_least_squares(m, n, rp, ci, va, delta, r1, r2)
    assert rc == o[5]
    for k in range(2):
        assert (H.st[k].niter, H.st[k].status) == (o[4][k].niter, o[4][k].status), k
    e = oracle.exact_two_least_squares(As, delta, r1, r2) if exact else o[:4]
    for got, want, alt, ex in zip((p1, q1, p2, q2), o[:4], ob2[:4], e):
        assert _rel(got, want) < max(1e-9, 20 * _rel(alt, want)) and _rel(got, ex) < 1e-3
    H.close()


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("delta", [SE, 0.25])
@pytest.mark.parametrize("kind", ORDER_SENSITIVE)
def test_order_sensitive_structures_stay_within_the_restatements_own_spread(oracle, kind, delta, fuse):
    """One dense row (a long row of A: a row group of its own), one dense column (a row of A' longer than an LDS stage:
    unpadded A', the long-row branch), columns of A without entries (empty row blocks of A').  On these three the
    Golub-Kahan vectors lose orthogonality in episodes -- device and restatement, equal to 1e-15 after one iteration, drift
    apart by x5 ... x1000 per iteration, come together again, drift again (profiles/r04_fixed_iteration_probe.txt, measured
    on the device with both programs cut at k = 1, 2, ... iterations; no jump at any k) -- and where an episode meets a
    stopping threshold, WHEN the test fires depends on rounding: the C restatement itself, run with its products summed left
    to right, right to left, or with the long rows in the device's order (oracle.set_sum_order; measured on the CPU by
    tests/test_oracle.py::test_iteration_counts_depend_on_the_summation_order_only_for_a_dominant_row_or_column), ends up to
    two iterations apart on the dense cases.  The device (whose every reduction associates differently, and whose compiler
    contracts other multiply-adds) must stay within ONE iteration of that spread, with the same statuses, and agree with the
    restatement's vectors as closely as the restatement's variants agree among themselves (1e-4).  That the layouts are
    right is shown iteration for iteration by the test above, and at the end by the one below."""
    H, As, m, n, (rp, ci, va), g, c, r1, r2 = _awkward_case(kind, delta, fuse)
    dev_m = (*H.solve_two_mixed(g, c)[:5], [(H.st[k].niter, H.st[k].status, H.st[k].solved) for k in range(2)])
    dev_l = (*H.solve_two_least_squares(r1, r2)[:5], [(H.st[k].niter, H.st[k].status, H.st[k].solved) for k in range(2)])
    H.close()
    var_m, var_l = [], []
    try:
        for mode in (0, 1, 2):
            oracle.set_sum_order(mode)
            var_m.append(oracle.solve_two_mixed(m, n, rp, ci, va, delta, g, c))
            var_l.append(oracle.solve_two_least_squares(m, n, rp, ci, va, delta, r1, r2))
    finally:
        oracle.set_sum_order(0)
    for dev, var in ((dev_m, var_m), (dev_l, var_l)):
        assert dev[4] == var[0][5]
        for k in range(2):
            its = [v[4][k].niter for v in var]
            assert min(its) - 1 <= dev[5][k][0] <= max(its) + 1, (k, dev[5][k], its)
            assert all((dev[5][k][1], dev[5][k][2]) == (v[4][k].status, v[4][k].solved) for v in var), k
        spread = max(_rel(a, b) for v in var[1:] for a, b in zip(v[:4], var[0][:4]))
        assert spread < 1e-4
        for got, want in zip(dev[:4], var[0][:4]):
            assert _rel(got, want) < 1e-4


@pytest.mark.parametrize("kind", ORDER_SENSITIVE)
def test_order_sensitive_structures_converge_to_the_exact_solve(oracle, kind):
    """What the two structures above cannot show iteration for iteration they show at the end: with the stopping tests
    tightened to 1e-15 (conditioning limits off) the device's LSQR / CRAIG run on, through the same long-row kernels, to the
    EXACT KKT solution -- 1e-9 of a direct solve of K.  A wrong entry, a dropped tail or a mis-ordered tile of a long row
    would show here, whatever rounding does to the iteration count."""
    delta = 0.25
    H, As, m, n, (rp, ci, va), g, c, r1, r2 = _awkward_case(kind, delta, 1, **TIGHT)
    p1, q1, p2, q2, rc = H.solve_two_mixed(g, c)
    assert rc == 0
    for got, ex in zip((p1, q1, p2, q2), oracle.exact_two_mixed(As, delta, g, c)):
        assert _rel(got, ex) < 1e-9
    p1, q1, p2, q2, rc = H.solve_two_least_squares(r1, r2)
    assert rc == 0
    for got, ex in zip((p1, q1, p2, q2), oracle.exact_two_least_squares(As, delta, r1, r2)):
        assert _rel(got, ex) < 1e-9
    H.close()


@pytest.mark.parametrize("ln_method", [0, 1])  # 1: LNLQ as the least-norm recurrence of objgrad (fpsq_options.ln_method)
@pytest.mark.parametrize("kind", ["tiny", "square-ish", "empty-columns", "dense-row", "dense-column", "wide-window"])
def test_fused_qp_entries_on_awkward_structures(oracle, kind, ln_method):
    """The fused device entries (fpsq_qp_objgrad / fpsq_qp_hprod: fast start, riding updates and scalar steps, speculative
    tail) on the same shapes, twice per model (first call, then with the run-ahead armed): fx / gx / ys and Hv follow the C
    restatement of objgrad! / hprod! (1e-4: see the seam test above), same return codes; with CRAIG and with LNLQ (ln_method = 1)
    as the least-norm recurrence of objgrad."""
    rng = np.random.default_rng(21)
    A = _random_structure(kind, rng)
    A.sort_indices()
    m, n = A.shape
    qp = problems._finish(kind, n, m, A.indptr.astype(np.int64), A.indices.astype(np.int64), np.ascontiguousarray(A.data), 7)
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.25, ln_method=ln_method)
    opts = oracle.default_options(n, m, ln_method=ln_method)
    v = rng.standard_normal(n)
    for t in range(2):
        x = qp.point(1 + t)
        gx, ys, hv = np.empty(n), np.empty(m), np.empty(n)
        fx, rc = dev.objgrad(x, gx=gx, ys=ys)
        o = oracle.qp_objgrad(qp, x, 1e3, 1.0, 0.25, opts=opts)
        assert rc == o["rc"] and abs(fx - o["fx"]) <= 1e-6 * max(1.0, abs(o["fx"]))
        assert _rel(gx, o["gx"]) < 1e-4 and _rel(ys, o["ys"]) < 1e-4
        rch = dev.hprod(v, hv, 2)
        oh = oracle.qp_hprod(qp, v, 1e3, 1.0, 0.25, opts=opts)
        assert rch == oh["rc"] and _rel(hv, oh["Hv"]) < 1e-4
        # Val(1): + the LSQR / MINRES lanes of solve_two_extras (their steps ride with leaders too)
        rch = dev.hprod(v, hv, 1)
        oh = oracle.qp_hprod(qp, v, 1e3, 1.0, 0.25, approx=1, opts=opts)
        assert rch == oh["rc"] and _rel(hv, oh["Hv"]) < 1e-4
    dev.close()


def test_solve_two_mixed_tight_tolerance_vs_exact(oracle):
    qp = _small_pde(seed=9)
    A = qp.scipy_csr()
    g = qp.qdiag * qp.x + qp.d
    c = A @ qp.x - qp.b
    for delta in (0.0, 1e-3):
        H = _Handle(A, delta=delta, **{**TIGHT, "ls_atol": 1e-13, "ls_rtol": 1e-13, "ls_axtol": 1e-13,
                                       "ls_btol": 1e-13, "ls_etol": 1e-13, "ln_atol": 1e-13, "ln_rtol": 1e-13,
                                       "ln_btol": 1e-13})
        p1, q1, p2, q2, rc = H.solve_two_mixed(g, c)
        assert rc == 0
        e = oracle.exact_two_mixed(A, delta, g, c)
        for got, want in zip((p1, q1, p2, q2), e):
            assert _rel(got, want) < 1e-10
        # K sol = rhs residuals
        r1 = np.linalg.norm(p1 + A.T @ q1 - g) / np.linalg.norm(g)
        r2 = np.linalg.norm(A @ p2 - delta * q2 - c) / np.linalg.norm(c)
        assert r1 < 1e-11 and r2 < 1e-11
        H.close()


@pytest.mark.parametrize("fuse", [0, 1])
def test_solve_two_least_squares_parity(oracle, fuse):
    qp = problems.random_eqqp(n=3000, m=300, per_row=24, seed=5)
    A = qp.scipy_csr()
    rng = np.random.default_rng(0)
    r1, r2 = rng.standard_normal(qp.n), rng.standard_normal(qp.n)
    H = _Handle(A, delta=0.01, fuse_two_rhs=fuse)
    p1, q1, p2, q2, rc = H.solve_two_least_squares(r1, r2)
    o = oracle.solve_two_least_squares(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, 0.01, r1, r2)
    assert rc == o[5] == 0
    for k in range(2):
        assert H.st[k].niter == o[4][k].niter and H.st[k].status == o[4][k].status
    e = oracle.exact_two_least_squares(A, 0.01, r1, r2)
    for got, want_c, want_e in zip((p1, q1, p2, q2), o[:4], e):
        assert _rel(got, want_c) < 1e-9 and _rel(got, want_e) < 1e-6
    H.close()


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("delta", [0.0, 0.01])
def test_solve_two_extras_parity(oracle, delta, fuse):
    """LSQR + MINRES on A A' + tau I (src/solve_linear_system.jl:45-77): iteration parity with the C restatement at
    the reference's default tolerances, and agreement with the exact solve.  fuse = 1: the MINRES recurrence runs as
    the second lane of the lock-step loop (its products share the LSQR lane's SpMMs); fuse = 0: one after the other.
    Repeated calls (the run-ahead history) and a zero second right-hand side give the same answers."""
    qp = problems.random_eqqp(n=3000, m=300, per_row=24, seed=5)
    A = qp.scipy_csr()
    rng = np.random.default_rng(1)
    r1, r2 = rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    H = _Handle(A, delta=delta, fuse_two_rhs=fuse)
    a, b, rc = H.solve_two_extras(r1, r2)
    o = oracle.solve_two_extras(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, r1, r2)
    assert rc == o[3]
    for k in range(2):
        assert H.st[k].niter == o[2][k].niter and H.st[k].status == o[2][k].status
        assert H.st[k].solved == o[2][k].solved
    assert H.st[0].niter > 5 and H.st[1].niter > 5
    ea, eb = oracle.exact_two_extras(A, delta, r1, r2)
    assert _rel(a, o[0]) < 1e-9 and _rel(b, o[1]) < 1e-9
    assert _rel(a, ea) < 1e-6 and _rel(b, eb) < 1e-6
    a2, b2, rc2 = H.solve_two_extras(r1, r2)  # second call: the host paces itself on the first call's counts
    assert rc2 == rc and np.array_equal(a, a2) and np.array_equal(b, b2)
    a3, b3, _ = H.solve_two_extras(1e-3 * r1, 0.0 * r2)  # hprod! Val(1) on a model with linear constraints: Ssv = 0
    o3 = oracle.solve_two_extras(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, 1e-3 * r1, 0.0 * r2)
    assert np.all(b3 == 0.0) and H.st[1].niter == 0 and H.st[1].solved == o3[2][1].solved == 1
    assert H.st[0].niter == o3[2][0].niter and _rel(a3, o3[0]) < 1e-9
    a4, b4, _ = H.solve_two_extras(r1, r2)
    assert np.array_equal(a, a4) and np.array_equal(b, b4)
    # tight tolerances: 1e-10 of the exact solution
    Ht = _Handle(A, delta=delta, ls_atol=1e-14, ls_rtol=1e-14, ls_axtol=1e-14, ls_btol=1e-14, ls_etol=1e-14,
                 ne_atol=1e-14, ne_rtol=1e-14, ne_etol=1e-14)
    a, b, rc = Ht.solve_two_extras(r1, r2)
    assert _rel(a, ea) < 1e-10 and _rel(b, eb) < 1e-9
    H.close()
    Ht.close()


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("delta", [0.0, SE, 0.25])
def test_lnlq_method_parity(oracle, delta, fuse):
    """fpsq_options.ln_method = FPSQ_LN_LNLQ: the least-norm system through LNLQ as the reference's generic
    solve_least_norm would run it with an LNLQ workspace (struct.jl:121, :251-281) -- lane for lane against the C
    restatement (niter, status, solved, vectors 1e-9), the minimum-norm solution of A x = -c for every delta, and the
    whole objgrad with the selector on."""
    qp = _small_pde(seed=19, n=4000, m=400)
    A = qp.scipy_csr()
    g = qp.qdiag * qp.x + qp.d
    c = A @ qp.x - qp.b
    H = _Handle(A, delta=delta, ln_method=1, fuse_two_rhs=fuse)
    p1, q1, p2, q2, rc = H.solve_two_mixed(g, c)
    o = oracle.solve_two_mixed(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, g, c,
                               oracle.default_options(qp.n, qp.m, ln_method=1))
    assert rc == o[5] == 0
    for k in range(2):
        assert (H.st[k].niter, H.st[k].status, H.st[k].solved) == (o[4][k].niter, o[4][k].status, o[4][k].solved)
    assert H.st[1].niter > 10 and H.st[1].status in (3, 9)
    for got, want in zip((p1, q1, p2, q2), o[:4]):
        assert _rel(got, want) < 1e-9
    Ad = A.toarray()
    ye = np.linalg.solve(Ad @ Ad.T, -c)
    assert _rel(q2, ye) < 1e-6 and _rel(p2, -(Ad.T @ ye)) < 1e-6  # delta only preconditions: unregularised answer
    p1b, q1b, p2b, q2b, _ = H.solve_two_mixed(g, c)  # run-ahead history
    assert np.array_equal(p2, p2b) and np.array_equal(q2, q2b) and np.array_equal(q1, q1b)
    z = H.solve_two_mixed(g, 0.0 * c)
    assert not z[2].any() and not z[3].any() and H.st[1].niter == 0 and H.st[1].solved == 1
    H.close()
    Hc = _Handle(A, delta=delta, ln_method=1, ln_itmax=3)
    Hc.solve_two_mixed(g, c)
    oc = oracle.solve_two_mixed(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, g, c,
                                oracle.default_options(qp.n, qp.m, ln_method=1, ln_itmax=3))
    assert (Hc.st[1].niter, Hc.st[1].status, Hc.st[1].solved) == (oc[4][1].niter, oc[4][1].status, oc[4][1].solved) == (4, 7, 0)
    Hc.close()
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta, ln_method=1, fuse_two_rhs=fuse)
    gx, ys = np.empty(qp.n), np.empty(qp.m)
    fx, rc = dev.objgrad(qp.x, gx=gx, ys=ys)
    od = oracle.qp_objgrad(qp, qp.x, 1e3, 1.0, delta, opts=oracle.default_options(qp.n, qp.m, ln_method=1))
    assert rc == od["rc"] == 0 and (dev.stats[0].niter, dev.stats[1].niter) == (od["stats"][0].niter, od["stats"][1].niter)
    assert _rel(gx, od["gx"]) < 1e-8 and _rel(ys, od["ys"]) < 1e-8 and abs(fx - od["fx"]) <= 1e-8 * abs(od["fx"])
    dev.close()


@pytest.mark.parametrize("delta", [0.0, SE, 0.25])
def test_minres_on_k_method_parity(oracle, delta):
    """fpsq_options.kkt_method = FPSQ_KKT_MINRES_K: both saddle-point systems by MINRES on K = [I A'; A -delta I] itself
    (named by BASELINE.json's north_star / configs[1]; NOT a path of the reference, so the checker is the generic MINRES
    restatement applied to K): niter / status / solved identical, vectors to 1e-9, the exact KKT solution to 1e-6 at the
    reference's sqrt(eps) tolerances and to 1e-11 at tight ones; fpsq_ys_gs through it; the fused QP entry refuses."""
    qp = _small_pde(seed=23, n=4000, m=400)
    A = qp.scipy_csr()
    g = qp.qdiag * qp.x + qp.d
    c = A @ qp.x - qp.b
    g2 = np.random.default_rng(2).standard_normal(qp.n)
    H = _Handle(A, delta=delta, kkt_method=1)
    p1, q1, p2, q2, rc = H.solve_two_mixed(g, c)
    w1 = oracle.minres_kkt(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, bp=g)
    w2 = oracle.minres_kkt(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, bq=c)
    assert rc == 0
    for k, w in enumerate((w1, w2)):
        assert (H.st[k].niter, H.st[k].status, H.st[k].solved) == (w[2].niter, w[2].status, w[2].solved)
        assert H.st[k].niter > 20 and H.st[k].solved == 1
    for got, want in zip((p1, q1, p2, q2), (w1[0], w1[1], w2[0], w2[1])):
        assert _rel(got, want) < 1e-9
    for got, want in zip((p1, q1, p2, q2), oracle.exact_two_mixed(A, delta, g, c)):
        assert _rel(got, want) < 1e-6
    # solve_two_least_squares: K [p; q] = [rhs; 0] twice
    a1, b1, a2, b2, rc = H.solve_two_least_squares(g, g2)
    w3 = oracle.minres_kkt(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, bp=g2)
    assert rc == 0 and H.st[1].niter == w3[2].niter
    assert _rel(a1, w1[0]) < 1e-9 and _rel(b1, w1[1]) < 1e-9 and _rel(a2, w3[0]) < 1e-9 and _rel(b2, w3[1]) < 1e-9
    # zero right-hand side: that lane ends at once, the other is unaffected
    z = H.solve_two_mixed(g, 0.0 * c)
    assert not z[2].any() and not z[3].any() and H.st[1].niter == 0 and H.st[1].solved == 1
    assert np.array_equal(z[0], p1) and np.array_equal(z[1], q1)
    H.close()
    Ht = _Handle(A, delta=delta, kkt_method=1, ne_atol=1e-14, ne_rtol=1e-14, ne_etol=1e-16)
    tight = Ht.solve_two_mixed(g, c)
    for got, want in zip(tight[:4], oracle.exact_two_mixed(A, delta, g, c)):
        assert _rel(got, want) < 1e-11
    Ht.close()
    Hi = _Handle(A, delta=delta, kkt_method=1, ne_itmax=5)
    Hi.solve_two_mixed(g, c)
    wi = oracle.minres_kkt(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, bp=g, itmax=5)
    assert (Hi.st[0].niter, Hi.st[0].status, Hi.st[0].solved) == (wi[2].niter, wi[2].status, wi[2].solved) == (5, 7, 0)
    Hi.close()
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta, kkt_method=1)
    gs, ys, v, w = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)
    assert dev.ys_gs(g, c, gs, ys, v, w) == 0
    assert _rel(ys, q1 + 1e3 * q2) < 1e-12 and _rel(gs, p1 + 1e3 * p2) < 1e-12
    with pytest.raises(Exception):
        dev.objgrad(qp.x, gx=np.empty(qp.n))
    dev.close()


def test_zero_right_hand_sides():
    """Edge cases of lsqr!/craig!: b = 0 returns x = 0, solved, 0 iterations."""
    qp = _small_pde(n=600, m=60)
    H = _Handle(qp.scipy_csr())
    p1, q1, p2, q2, rc = H.solve_two_mixed(np.zeros(qp.n), np.zeros(qp.m))
    assert rc == 0 and H.st[0].niter == 0 and H.st[1].niter == 0
    assert H.st[0].status == 1 and H.st[1].status == 1
    assert not p1.any() and not q1.any() and not p2.any() and not q2.any()
    H.close()


def test_itmax_reports_unsolved_softly():
    """Numerical failure is a soft return code (the reference only @warns), never an exception."""
    qp = _small_pde(n=600, m=60)
    A = qp.scipy_csr()
    H = _Handle(A, ls_itmax=2, ln_itmax=2)
    g = qp.qdiag * qp.x + qp.d
    c = A @ qp.x - qp.b
    *_, rc = H.solve_two_mixed(g, c)
    assert rc == 3 and H.st[0].niter == 2 and H.st[1].niter == 2 and H.st[0].status == 7 and H.st[1].status == 7
    H.close()


# ---------------------------------------------------------------------------------------------- penalty gradient

@pytest.mark.parametrize("delta,eta", [(0.0, 0.0), (SE, 0.0), (1e-2, 0.5)])
def test_device_qp_objgrad_matches_oracle(oracle, delta, eta):
    qp = _small_pde(seed=11, n=3000, m=300)
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta, eta=eta)
    gx, ys, gs = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
    xk = qp.xhat.copy()
    fx, rc = dev.objgrad(qp.x, gx=gx, ys=ys, gs=gs, xk=xk if eta > 0 else None)
    o = oracle.qp_objgrad(qp, qp.x, 1e3, 1.0, delta, eta, xk)
    assert rc == o["rc"] == 0
    assert dev.stats[0].niter == o["stats"][0].niter and dev.stats[1].niter == o["stats"][1].niter
    # same algorithm, same tolerances: differences are summation-order rounding amplified by sigma = 1e3
    assert _rel(ys, o["ys"]) < 1e-8 and _rel(gs, o["gs"]) < 1e-8 and _rel(gx, o["gx"]) < 1e-8
    assert abs(fx - o["fx"]) <= 1e-8 * abs(o["fx"])
    e = oracle.exact_qp_objgrad(qp, qp.x, 1e3, 1.0, delta, eta, xk)
    assert _rel(ys, e["ys"]) < 1e-5 and _rel(gx, e["gx"]) < 1e-5
    dev.close()


def test_device_qp_matches_host_mirror(oracle):
    """The device-resident evaluation and FletcherPenaltyNLP + HIPQDSolver with a host model agree."""
    qp = _small_pde(seed=13, n=2000, m=200)
    model = nlpmodels.EqQPModel(qp)
    fp = FletcherPenaltyNLP(model, 1e3, 1.0, SE, 2, qds=HIPQDSolver(model, 0.0))
    f_host, g_host = fp.objgrad(qp.x)
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=SE)
    g_dev = np.empty(qp.n)
    f_dev, rc = dev.objgrad(qp.x, gx=g_dev)
    assert rc == 0
    assert _rel(g_dev, g_host) < 1e-9 and abs(f_dev - f_host) <= 1e-9 * abs(f_host)
    dev.close()
    fp.qdsolver.close()


@pytest.mark.parametrize("delta,rho,eta", [(0.0, 1.0, 0.0), (SE, 0.0, 0.0), (1e-2, 2.0, 0.5)])
def test_device_qp_hprod_matches_host_mirror(delta, rho, eta):
    """fpsq_qp_hprod (device-resident hprod! Val(2)) against the host mirror of src/model-Fletcherpenaltynlp.jl:521-570
    driven through the same back-end; the penalty Hessian approximation is symmetric to the Krylov tolerance."""
    qp = _small_pde(seed=31, n=3000, m=300)
    dev = DeviceEqQP(qp, sigma=1e3, rho=rho, delta=delta, eta=eta, **TIGHT)
    model = nlpmodels.EqQPModel(qp)
    qds = HIPQDSolver(model, 0.0, **TIGHT)
    fp = FletcherPenaltyNLP(model, sigma=1e3, rho=rho, delta=delta, hessian_approx=2, qds=qds)
    fp.eta = eta
    rng = np.random.default_rng(5)
    v, w = rng.standard_normal(qp.n), rng.standard_normal(qp.n)
    Hv, Hw = np.empty(qp.n), np.empty(qp.n)
    assert dev.hprod(v, Hv) == 0 and dev.hprod(w, Hw) == 0
    want = fp.hprod(qp.x, v)
    assert _rel(Hv, want) < 1e-9
    assert abs(w @ Hv - v @ Hw) <= 1e-7 * (np.linalg.norm(w) * np.linalg.norm(Hv))
    dev.close()
    qds.close()


@pytest.mark.parametrize("delta,rho,eta", [(0.0, 1.0, 0.0), (SE, 0.0, 0.0), (1e-2, 2.0, 0.5)])
def test_device_qp_hprod_matches_oracle(oracle, delta, rho, eta):
    """fpsq_qp_hprod against the C restatement of hprod! Val(2) (oracle fpo_qp_hprod, model-Fletcherpenaltynlp.jl:521-570)
    at the reference's default tolerances: same LSQR iteration counts / status, Hv to 1e-8; and, at tight tolerances,
    against the exact KKT solve to 1e-9."""
    qp = _small_pde(seed=31, n=3000, m=300)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(qp.n)
    dev = DeviceEqQP(qp, sigma=1e3, rho=rho, delta=delta, eta=eta)
    Hv = np.empty(qp.n)
    rc = dev.hprod(v, Hv)
    o = oracle.qp_hprod(qp, v, 1e3, rho, delta, eta)
    assert rc == o["rc"] == 0
    for k in range(2):
        assert (dev.stats[k].niter, dev.stats[k].status, dev.stats[k].solved) == \
               (o["stats"][k].niter, o["stats"][k].status, o["stats"][k].solved)
    assert dev.stats[0].niter > 10
    assert _rel(Hv, o["Hv"]) < 1e-8
    dev.close()
    dev = DeviceEqQP(qp, sigma=1e3, rho=rho, delta=delta, eta=eta, **TIGHT)
    assert dev.hprod(v, Hv) == 0
    assert _rel(Hv, oracle.exact_qp_hprod(qp, v, 1e3, rho, delta, eta)) < 1e-9
    dev.close()


@pytest.mark.parametrize("delta,rho,eta", [(0.0, 1.0, 0.0), (SE, 0.0, 0.0), (1e-2, 2.0, 0.5)])
def test_device_qp_hprod_val1_matches_oracle_and_host_mirror(oracle, delta, rho, eta):
    """fpsq_qp_hprod with hessian_approx = 1 (hprod! Val(1), model-Fletcherpenaltynlp.jl:572-634) against the C restatement
    (fpo_qp_hprod, approx = 1): the statistics of all FOUR recurrences (two LSQR of solve_two_least_squares, LSQR + MINRES of
    solve_two_extras with tau = max(delta, 1e-14) and the zero right-hand side Ssv), Hv to 1e-8; against the host mirror of
    the reference's Val(1) driven through the iterative back-end; and -- the constraint Hessians vanish -- equal to Val(2)'s
    product bit for bit."""
    qp = _small_pde(seed=31, n=3000, m=300)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(qp.n)
    dev = DeviceEqQP(qp, sigma=1e3, rho=rho, delta=delta, eta=eta)
    Hv1, Hv2 = np.empty(qp.n), np.empty(qp.n)
    rc = dev.hprod(v, Hv1, 1)
    o = oracle.qp_hprod(qp, v, 1e3, rho, delta, eta, approx=1)
    assert rc == o["rc"]
    for k in range(4):
        got, want = dev.stats4[k], o["stats"][k]
        assert (got.niter, got.status, got.solved) == (want.niter, want.status, want.solved), k
    assert dev.stats4[2].niter > 10 and dev.stats4[3].status == 1  # MINRES on the zero right-hand side: "x = 0 ..."
    assert _rel(Hv1, o["Hv"]) < 1e-8
    assert dev.hprod(v, Hv2, 2) == 0
    assert np.array_equal(Hv1, Hv2)
    # a device-resident argument pair takes the in-place path
    import torch
    vt, ht = torch.from_numpy(v).cuda(), torch.empty(qp.n, dtype=torch.float64, device="cuda")
    assert dev.hprod(vt, ht, 1) == rc and np.array_equal(ht.cpu().numpy(), Hv1)
    dev.close()
    model = nlpmodels.EqQPModel(qp)
    qds = HIPQDSolver(model, 0.0, **TIGHT)
    fp = FletcherPenaltyNLP(model, sigma=1e3, rho=rho, delta=delta, hessian_approx=1, qds=qds)
    fp.eta = eta
    dev = DeviceEqQP(qp, sigma=1e3, rho=rho, delta=delta, eta=eta, **TIGHT)
    assert dev.hprod(v, Hv1, 1) == 0
    assert _rel(Hv1, fp.hprod(qp.x, v)) < 1e-9
    dev.close()
    qds.close()


@pytest.mark.parametrize("delta", [0.0, SE, 1e-2])
def test_device_qp_hprod_val1_shortcuts_are_bitwise_the_full_computation(monkeypatch, delta):
    """hprod! Val(1) of the equality-QP model: the MINRES lane of solve_two_extras has a zero right-hand side (J' of its zero
    solution is not formed), and for delta >= 1e-14 its LSQR lane repeats the first solve of solve_two_least_squares bit for
    bit (statistics taken from there).  FPSQ_AB_MASK bit 16 computes everything: Hv and all four recurrences' statistics
    must be identical."""
    qp = _small_pde(seed=37, n=5000, m=500)
    rng = np.random.default_rng(9)
    monkeypatch.setenv("FPSQ_AB_MASK", "16")
    full = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
    monkeypatch.setenv("FPSQ_AB_MASK", "0")
    fast = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
    for k in range(3):
        v = rng.standard_normal(qp.n)
        res = []
        for mdl in (full, fast):
            hv = np.empty(qp.n)
            rc = mdl.hprod(v, hv, 1)
            st = [(s_.niter, s_.status, s_.solved, s_.rnorm, s_.arnorm) for s_ in (mdl.stats4[i] for i in range(4))]
            res.append((rc, hv, st))
        assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2], k
    full.close()
    fast.close()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("delta", [0.0, SE, 0.25])
def test_ys_gs_entry_point(oracle, where, delta):
    """fpsq_ys_gs, the fused `_compute_ys_gs!` convenience of the boundary (model-Fletcherpenaltynlp.jl:242-248), with
    host and with device pointers: gs = p1 + sigma p2, ys = q1 + sigma q2, v = p2, w = q2 of fpsq_solve_two_mixed on the
    same right-hand sides (v, w bitwise: same kernels, same order), and ys / gs of the C restatement's objgrad! to 1e-8."""
    import torch

    qp = _small_pde(seed=17, n=4000, m=400)
    sigma = 1e3
    dev = DeviceEqQP(qp, sigma=sigma, rho=1.0, delta=delta)
    A = qp.scipy_csr()
    g = qp.qdiag * qp.x + qp.d
    c = A @ qp.x - qp.b
    p1, q1, p2, q2 = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)
    rc_mixed = dev.solve_two_mixed(g, c, p1, q1, p2, q2)
    its = (dev.stats[0].niter, dev.stats[1].niter)
    if where == "host":
        gs, ys, v, w = np.full(qp.n, np.nan), np.full(qp.m, np.nan), np.full(qp.n, np.nan), np.full(qp.m, np.nan)
        rc = dev.ys_gs(g, c, gs, ys, v, w)
    else:
        tg, tc = torch.from_numpy(g).cuda(), torch.from_numpy(c).cuda()
        outs = [torch.full((k,), float("nan"), dtype=torch.float64, device="cuda") for k in (qp.n, qp.m, qp.n, qp.m)]
        torch.cuda.synchronize()
        rc = dev.ys_gs(tg, tc, *outs)
        gs, ys, v, w = [t.cpu().numpy() for t in outs]
    assert rc == rc_mixed and (dev.stats[0].niter, dev.stats[1].niter) == its
    assert np.array_equal(v, p2) and np.array_equal(w, q2)
    # (the device contracts a + sigma * b into one fma: one rounding of difference at most)
    assert np.all(np.abs(gs - (p1 + sigma * p2)) <= 4e-16 * (np.abs(p1) + sigma * np.abs(p2)))
    assert np.all(np.abs(ys - (q1 + sigma * q2)) <= 4e-16 * (np.abs(q1) + sigma * np.abs(q2)))
    o = oracle.qp_objgrad(qp, qp.x, sigma, 1.0, delta)
    assert rc == o["rc"] and its == (o["stats"][0].niter, o["stats"][1].niter)
    assert _rel(ys, o["ys"]) < 1e-8 and _rel(gs, o["gs"]) < 1e-8
    dev.close()


def test_device_inputs_are_ordered_after_the_producer_stream(oracle):
    """include/fpsq.h "INPUT READINESS": the library runs on its own non-blocking stream and reads device tensors in
    place, so the evaluation must wait for the torch kernels that are still PRODUCING x when the call is made.  Here x
    is far from its final value until a queue of ~2 ms of torch work (a large matmul, then 50 in-place updates) has
    run; objgrad is called right behind it with no host synchronisation and must see the final x (n = 1e6)."""
    import torch

    qp = problems.pde_control_like(n=1_000_000, m=100_000)
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
    x0 = torch.from_numpy(qp.point(5)).cuda()
    noise = torch.from_numpy(qp.point(6) - qp.xhat).cuda()
    big = torch.randn(4096, 4096, dtype=torch.float64, device="cuda")
    gx = torch.empty(qp.n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for rep in range(3):
        x = x0 + 50.0 * noise          # far away (phi differs by orders of magnitude)
        _ = big @ big                  # ~2 ms of queued work ahead of the updates
        for _k in range(50):
            x.sub_(noise)              # ... ends at x0 exactly? no: at x0 + 50 noise - 50 noise up to rounding
        fx, rc = dev.objgrad(x, gx=gx)  # no torch.cuda.synchronize() in between
        xh = x.cpu().numpy()           # the final x, read back AFTER the call
        o = oracle.qp_objgrad(qp, xh, 1e3, 1.0, 0.0)
        assert rc == o["rc"] == 0
        assert (dev.stats[0].niter, dev.stats[1].niter) == (o["stats"][0].niter, o["stats"][1].niter)
        assert abs(fx - o["fx"]) <= 1e-8 * abs(o["fx"])
        assert _rel(gx.cpu().numpy(), o["gx"]) < 1e-8
    dev.close()


def test_torch_device_pointers_accepted():
    import torch

    qp = _small_pde(seed=15, n=2000, m=200)
    dev = DeviceEqQP(qp)
    x = torch.from_numpy(qp.x).cuda()
    gx = torch.empty(qp.n, dtype=torch.float64, device="cuda")
    fx, rc = dev.objgrad(x, gx=gx)
    torch.cuda.synchronize()
    g2 = np.empty(qp.n)
    fx2, _ = dev.objgrad(qp.x, gx=g2)
    assert rc == 0 and fx == fx2 and np.array_equal(gx.cpu().numpy(), g2)
    dev.close()


def test_repeat_calls_are_bitwise_reproducible():
    qp = _small_pde(seed=17, n=3000, m=300)
    dev = DeviceEqQP(qp, delta=SE)
    a, b = np.empty(qp.n), np.empty(qp.n)
    f1, _ = dev.objgrad(qp.x, gx=a)
    dev.objgrad(qp.point(1), gx=b)
    f2, _ = dev.objgrad(qp.x, gx=b)
    assert f1 == f2 and np.array_equal(a, b)
    dev.close()


def test_run_ahead_history_does_not_change_results(oracle):
    """The host holds its run-ahead at the iteration count of the previous call of the same kind; a wrong guess in
    either direction (easy problem after a hard one and back) must give exactly what a fresh handle gives."""
    qp = _small_pde(seed=23, n=4000, m=400)
    A = qp.scipy_csr()
    g = qp.qdiag * qp.x + qp.d
    c = A @ qp.x - qp.b
    easy = 1e-3 * g  # stops after fewer iterations under the absolute tolerance
    H = _Handle(A, delta=0.0)
    seq = [(g, c), (easy, 1e-3 * c), (g, c), (g, 0.0 * c), (g, c)]
    its = []
    for r1, r2 in seq:
        got = H.solve_two_mixed(r1, r2)
        its.append((H.st[0].niter, H.st[1].niter))
        F = _Handle(A, delta=0.0)
        want = F.solve_two_mixed(r1, r2)
        assert (F.st[0].niter, F.st[1].niter) == its[-1]
        for a, b in zip(got[:4], want[:4]):
            assert np.array_equal(a, b)
        F.close()
    assert len(set(its)) >= 2, its  # the sequence really changes the iteration counts
    H.close()


def test_speculative_epilogue_is_bitwise_neutral(monkeypatch):
    """objgrad / hprod enqueue their epilogue speculatively behind the iteration count of the PREVIOUS call (gated on the
    recurrences' `done` flags).  Over a sequence of points whose Krylov counts go up and down (misses in both
    directions, one lane ending before the other), results must be bitwise those of a handle with the adaptive
    run-ahead switched off -- in particular the final LSQR update is applied exactly once."""
    import torch

    tight = dict(TIGHT)
    qp = _small_pde(seed=5, n=3000, m=300)
    monkeypatch.setenv("FPSQ_ADAPTIVE_RUNAHEAD", "0")
    ref = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0, **tight)
    monkeypatch.setenv("FPSQ_ADAPTIVE_RUNAHEAD", "1")
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0, **tight)
    rng = np.random.default_rng(0)
    counts = set()
    for k in range(40):
        scale = 0.5 ** (k % 14) * (1.0 if k % 3 else 1e-3)
        x = qp.xhat + scale * rng.standard_normal(qp.n)
        g1, g2, y1, y2 = np.empty(qp.n), np.empty(qp.n), np.empty(qp.m), np.empty(qp.m)
        f1, rc1 = ref.objgrad(x, gx=g1, ys=y1)
        i1 = (ref.stats[0].niter, ref.stats[1].niter)
        if k % 2:  # device-resident arguments take the in-place path
            xt = torch.from_numpy(x).cuda()
            t2 = torch.empty(qp.n, dtype=torch.float64, device="cuda")
            f2, rc2 = dev.objgrad(xt, gx=t2, ys=y2)
            g2 = t2.cpu().numpy()
        else:
            f2, rc2 = dev.objgrad(x, gx=g2, ys=y2)
        assert (dev.stats[0].niter, dev.stats[1].niter) == i1 and rc1 == rc2
        assert f1 == f2 and np.array_equal(g1, g2) and np.array_equal(y1, y2), (k, i1)
        counts.add(i1)
        if k % 5 == 0:
            v = scale * rng.standard_normal(qp.n)
            h1, h2 = np.empty(qp.n), np.empty(qp.n)
            assert ref.hprod(v, h1) == dev.hprod(v, h2)
            assert np.array_equal(h1, h2)
    assert len(counts) >= 4, counts  # the sequence really moves the iteration counts around
    ref.close()
    dev.close()


@pytest.mark.parametrize("delta", [0.0, SE])
def test_speculative_epilogue_every_alignment_is_bitwise_neutral(delta):
    """The same property, deterministically: fpsq_debug_expect_iterations places the speculation (gated final LSQR update +
    gated epilogue kernels) at EVERY position relative to the true iteration counts of the two lanes -- before the first
    lane ends, between the two ends, exactly at the last end (the hit), behind it -- for objgrad (LSQR + CRAIG lanes, the
    paired two-RHS epilogue product), hprod (two LSQR lanes, the single-RHS epilogue products), solve_two_mixed and
    solve_two_least_squares (no caller epilogue).  Every result must be bitwise the one of a handle that never speculates
    (round 2 saw an intermittent mismatch in the hprod leg with an experimental A' kernel that also replaced the single-RHS
    instantiation only that leg runs; this test pins the kept host logic independently of timing)."""
    qp = _small_pde(seed=7, n=3000, m=300)
    ref = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
    lib = dev._lib
    rng = np.random.default_rng(1)
    x = qp.xhat + 0.3 * rng.standard_normal(qp.n)
    v = rng.standard_normal(qp.n)
    g, c = qp.qdiag * x + qp.d, qp.scipy_csr() @ x - qp.b

    def run(model, which):
        if which == "objgrad":
            gx, ys = np.empty(qp.n), np.empty(qp.m)
            f, rc = model.objgrad(x, gx=gx, ys=ys)
            return (np.array([f]), gx, ys), rc
        if which == "hprod":
            hv = np.empty(qp.n)
            return (hv,), model.hprod(v, hv)
        o = [np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)]
        rc = model.solve_two_mixed(g, c, *o) if which == "mixed" else model.solve_two_least_squares(g, v, *o)
        return tuple(o), rc

    for which in ("objgrad", "hprod", "mixed", "lsq"):
        lib.fpsq_debug_expect_iterations(ref._h, 0)  # never speculates
        want, rc0 = run(ref, which)
        its = (ref.stats[0].niter, ref.stats[1].niter)
        assert min(its) >= 2, its
        for e in range(0, max(its) + 4):
            assert lib.fpsq_debug_expect_iterations(dev._h, e) == 0
            got, rc = run(dev, which)
            assert rc == rc0 and (dev.stats[0].niter, dev.stats[1].niter) == its, (which, e)
            for a_, b_ in zip(want, got):
                assert np.array_equal(a_, b_), (which, e, its)
    ref.close()
    dev.close()


def test_column_phase_order_of_the_row_groups_is_a_reordering_only(oracle, monkeypatch):
    """The entries of a row group of the A-product layout are stored sorted by column PHASE, (col mod P) -- a rotation of the
    group's column order that lets all resident groups sweep the same absolute columns at the same time (the x window is
    then served by the L2 instead of being fetched again).  Any order of a group's entries is valid: against a handle with
    the plain column order (FPSQ_RGCS_PHASE=0) the plain products agree to rounding (different tiles, so different
    summation orders: 1e-13), the recurrences take the same number of iterations and objgrad agrees to 1e-9 -- and both
    with the C restatement as before."""
    qp = _small_pde(seed=17, n=60000, m=6000)
    monkeypatch.setenv("FPSQ_RGCS_PHASE", "0")
    ref = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
    monkeypatch.setenv("FPSQ_RGCS_PHASE", "1")
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
    rng = np.random.default_rng(4)
    A = qp.scipy_csr()
    x = qp.xhat + 0.3 * rng.standard_normal(qp.n)
    ys_ = []
    for mdl in (ref, dev):
        y = np.zeros(qp.m)
        mdl.jac_mul(False, 1.0, x, 0.0, y)
        ys_.append(y)
    want = A @ x
    assert _rel(ys_[0], want) < 1e-13 and _rel(ys_[1], want) < 1e-13
    out = []
    for mdl in (ref, dev):
        gx, ys = np.empty(qp.n), np.empty(qp.m)
        f, rc = mdl.objgrad(x, gx=gx, ys=ys)
        out.append((f, rc, gx, ys, mdl.stats[0].niter, mdl.stats[1].niter))
    assert out[0][1] == out[1][1] and out[0][4:] == out[1][4:]
    assert abs(out[0][0] - out[1][0]) <= 1e-9 * abs(out[0][0]) and _rel(out[0][2], out[1][2]) < 1e-9 and _rel(out[0][3], out[1][3]) < 1e-9
    o = oracle.qp_objgrad(qp, x, 1e3, 1.0, 0.0)
    assert out[1][1] == o["rc"] and _rel(out[1][2], o["gx"]) < 1e-6
    ref.close()
    dev.close()


@pytest.mark.parametrize("shared", ["0", "1"])
@pytest.mark.parametrize("lead", ["0", "1"])
@pytest.mark.parametrize("delta", [0.0, SE])
def test_column_sorted_at_blocks_are_bitwise_the_row_order_layout(monkeypatch, delta, lead, shared):
    """A' of a banded Jacobian is stored with every row block's entries sorted by COLUMN (coalesced gathers: the row-order
    gather is what bounded the A' product), each entry carrying its row-major slot, to which its product is scattered
    (k_spmv<.., CSORT>).  Same values summed in the same order: every output must be BITWISE that of a handle storing the
    blocks in row order (FPSQ_AT_SORTED=0) -- objgrad, hprod (both Hessian approximations), the seam solves, the one-lane
    kernels of an unfused handle, with the scalar steps riding in the products (leader workgroups) and without.
    shared = 1 (the default since round 4): the blocks hold NO values of their own -- every entry is read from the row-group
    copy of A through segment descriptors (fpsq_layout.h pad_blocks, "shared values"): the entries stream in another order
    again, into the same LDS slots."""
    qp = _small_pde(seed=13, n=30000, m=3000)
    monkeypatch.setenv("FPSQ_RIDE_LEAD", lead)
    monkeypatch.setenv("FPSQ_AT_SHARED", shared)
    monkeypatch.setenv("FPSQ_AT_SORTED", "0")
    ref = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
    one_ref = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta, fuse_two_rhs=0)
    monkeypatch.setenv("FPSQ_AT_SORTED", "1")
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
    one = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta, fuse_two_rhs=0)
    want = 2 if shared == "1" else 1
    assert ref.info()["at_sorted"] == 0 and dev.info()["at_sorted"] == want and one.info()["at_sorted"] == want
    rng = np.random.default_rng(3)
    A = qp.scipy_csr()
    for k in range(4):
        x = qp.xhat + 0.3 * 0.5 ** k * rng.standard_normal(qp.n)
        v = rng.standard_normal(qp.n)
        res = []
        for mdl in (ref, dev, one_ref, one):
            gx, ys, gs, hv = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.n)
            f, rc = mdl.objgrad(x, gx=gx, ys=ys, gs=gs)
            rch = mdl.hprod(v, hv, 1 + k % 2)
            o = [np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)]
            rcm = mdl.solve_two_mixed(qp.qdiag * x + qp.d, A @ x - qp.b, *o)
            res.append([np.array([f, rc, rch, rcm]), gx, ys, gs, hv, *o])
        for i, j in ((0, 1), (2, 3)):
            for a_, b_ in zip(res[i], res[j]):
                assert np.array_equal(a_, b_), (k, i)
    for mdl in (ref, dev, one, one_ref):
        mdl.close()


@pytest.mark.parametrize("size", [(6000, 600), (300000, 30000)])
@pytest.mark.parametrize("delta", [0.0, SE])
def test_steps_riding_with_leaders_are_bitwise_the_stand_alone_steps(monkeypatch, delta, size):
    """Large product grids hand the scalar steps to two LEADER workgroups at the head of the next product launch
    (k_spmv_atl / k_spmv_rgcs<.., LEAD>: the step computed once, published behind a device-scope release, picked up by the
    other workgroups on their way to the row epilogue; whoever finds nothing recomputes it).  Same step code on the same
    inputs: every output and every statistic must be BITWISE those of a handle with FPSQ_RIDE_LEAD=0 (stand-alone k_step
    launches) -- small grids (all workgroups resident at once, most of them ahead of the leaders) and a grid of several
    resident sets, objgrad / hprod / the seam solves, first calls and armed run-ahead."""
    n, m = size
    qp = _small_pde(seed=11, n=n, m=m)
    monkeypatch.setenv("FPSQ_RIDE_LEAD", "0")
    ref = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
    monkeypatch.setenv("FPSQ_RIDE_LEAD", "1")
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
    rng = np.random.default_rng(2)
    A = qp.scipy_csr()
    for k in range(6):
        scale = 0.5 ** (k % 5) * (1.0 if k % 3 else 1e-2)
        x = qp.xhat + scale * rng.standard_normal(qp.n)
        v = scale * rng.standard_normal(qp.n)
        want = None
        for mdl in (ref, dev):
            gx, ys, gs, hv = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.n)
            f, rc = mdl.objgrad(x, gx=gx, ys=ys, gs=gs)
            st = [(mdl.stats[i].niter, mdl.stats[i].status, mdl.stats[i].solved, mdl.stats[i].rnorm, mdl.stats[i].arnorm) for i in range(2)]
            rch = mdl.hprod(v, hv, 1 + k % 2)
            # (Val(1): + the LSQR and MINRES lanes of solve_two_extras, whose steps ride too)
            sth = [(mdl.stats4[i].niter, mdl.stats4[i].status, mdl.stats4[i].rnorm) for i in range(4 if k % 2 == 0 else 2)]
            o = [np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)]
            rcm = mdl.solve_two_mixed(qp.qdiag * x + qp.d, A @ x - qp.b, *o)
            out = [np.array([f, rc, rch, rcm]), gx, ys, gs, hv, *o, np.array(st, dtype=float).ravel(), np.array(sth, dtype=float).ravel()]
            if mdl is ref:
                want = out
        for a_, b_ in zip(out, want):
            assert np.array_equal(a_, b_), k
    ref.close()
    dev.close()


@pytest.mark.parametrize("late", [0, 8, 3, 13])
def test_a_late_leader_changes_nothing(monkeypatch, late):
    """Sixteen leaders compute the riding steps redundantly and any of them may start late (another kernel holding its XCD).
    The riding UPDATE workgroups of the same launch are released by the record of their own XCC's leader alone, so whatever
    they write must not be an input of the step the late leader is still to compute: the update partials alternate between
    two arrays (fpsq_handle.hip.h: pW / pWalt).  FPSQ_DEBUG_RIDE_DELAY=c+1 holds leader c of every launch back by ~100 us -- a
    committing leader (0: lane 0, 8: lane 1) or a publishing-only one -- and every output and statistic of objgrad, hprod
    Val(1) / Val(2), solve_two_mixed and solve_two_extras (the MINRES lane: beta = sqrt of a sum of those partials) must stay
    BITWISE that of a handle with stand-alone step launches (FPSQ_RIDE_LEAD=0)."""
    qp = _small_pde(seed=13, n=60000, m=6000)
    A = qp.scipy_csr()
    rng = np.random.default_rng(4)
    xs = [qp.xhat + 0.3 * rng.standard_normal(qp.n) for _ in range(3)]
    r2 = [rng.standard_normal(qp.m) for _ in range(3)]

    def run():
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
        raw = _Handle(A, 0.0)
        out = []
        for k, x in enumerate(xs):
            gx, ys, hv = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
            f, rc = dev.objgrad(x, gx=gx, ys=ys)
            rch = dev.hprod(x, hv, 1 + k % 2)
            st = [(dev.stats4[i].niter, dev.stats4[i].status, dev.stats4[i].rnorm) for i in range(2)]
            e1, e2, rce = raw.solve_two_extras(x, r2[k])
            ste = [(raw.st[i].niter, raw.st[i].status, raw.st[i].rnorm, raw.st[i].arnorm) for i in range(2)]
            out += [np.array([f, rc, rch, rce]), gx, ys, hv, e1, e2, np.array(st).ravel(), np.array(ste).ravel()]
        dev.close()
        raw.close()
        return out

    monkeypatch.setenv("FPSQ_RIDE_LEAD", "0")
    want = run()
    monkeypatch.setenv("FPSQ_RIDE_LEAD", "1")
    monkeypatch.setenv("FPSQ_DEBUG_RIDE_DELAY", str(late + 1))
    got = run()
    assert got[0][3] >= 0 and want[6].size == 6  # (the MINRES lane iterated: niter of lane 1 of the extras call)
    assert int(want[7][4]) > 3
    for i, (a_, b_) in enumerate(zip(got, want)):
        assert np.array_equal(a_, b_), i


@pytest.mark.parametrize("size", [(6000, 600), (60000, 6000), (300000, 30000), (300000, 30000, "headline density")])
@pytest.mark.parametrize("delta", [0.0, SE])
def test_one_launch_iterations_are_bitwise_the_two_launch_iterations(monkeypatch, delta, size):
    """A joint iteration of two riding recurrences is ONE launch (k_iter_fused): the row groups of the A product follow the
    A' blocks in the same grid and start when the blocks owning what they gather have published themselves (written-through
    rows, per-block flags, agent-scope gathers), the steps behind the A' product are computed by a second set of leaders from
    tagged partials.  Same per-block and per-group arithmetic, the same sums in the same order: every output and statistic
    of objgrad, hprod Val(2) and the seam solves must be BITWISE those of a handle that launches the two products separately
    on the same layout (FPSQ_FUSE_ITER=0 with the A' blocks aligned to 8 rows all the same), over changing points -- the
    second and later calls also exercise the run-ahead, the speculative epilogue and launches past convergence.
    "headline density" (100 entries per row in an 8192-column window, ~205-row A' blocks, several resident sets): blocks
    there reach their epilogue with the leaders' record taken at the LAST of their looks, which the sparser cases never do
    (an experimental build -- tools/experiments/ln_update_in_at_blocks.patch -- that mishandled that look passed the three
    other sizes and left half the rows of p2 wrong at this one)."""
    qp = _small_pde(seed=17, n=size[0], m=size[1]) if len(size) == 2 else problems.pde_control_like(n=size[0], m=size[1], seed=31)
    A = qp.scipy_csr()
    rng = np.random.default_rng(8)
    xs = [qp.xhat + 0.3 * 0.6 ** k * rng.standard_normal(qp.n) for k in range(5)]
    vs = [rng.standard_normal(qp.n) for _ in range(5)]

    def run(expect_fused):
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
        out, fused = [], 0
        for k, x in enumerate(xs):
            gx, ys, gs, hv = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.n)
            f, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs)
            fused += dev.info()["last_fused_launches"]
            st = [(dev.stats[i].niter, dev.stats[i].status, dev.stats[i].rnorm, dev.stats[i].arnorm) for i in range(2)]
            rch = dev.hprod(vs[k], hv, 2)
            o = [np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)]
            rcm = dev.solve_two_mixed(qp.qdiag * x + qp.d, A @ x - qp.b, *o)
            out += [np.array([f, rc, rch, rcm]), gx, ys, gs, hv, *o, np.array(st).ravel()]
        dev.close()
        assert (fused > 0) == expect_fused, fused
        return out

    monkeypatch.setenv("FPSQ_AT_ROW_ALIGN", "8")
    monkeypatch.setenv("FPSQ_FUSE_ITER", "0")
    want = run(False)
    monkeypatch.setenv("FPSQ_FUSE_ITER", "2")  # (2: wherever possible; the default, 1, keeps small grids on two launches)
    got = run(True)
    for i, (a_, b_) in enumerate(zip(got, want)):
        assert np.array_equal(a_, b_), i


@pytest.mark.parametrize("kmax", [2, 3, 8])
@pytest.mark.parametrize("size,delta", [((60000, 6000), 0.0), ((300000, 30000, "headline density"), 0.0),
                                        ((300000, 30000, "headline density"), SE)])
def test_several_iterations_per_launch_are_bitwise_one_iteration_per_launch(monkeypatch, kmax, size, delta):
    """k_iter_multi (csrc/fpsq_multi.hip.h): up to `kmax` joint iterations share ONE launch -- the A' blocks of iteration j + 1 start
    when the row groups of iteration j that wrote what they gather have published themselves, the recurrence state travels from
    leader set to leader set as self-validating words, the long pair alternates between two buffers.  Per block, per group, per
    update workgroup and per step the arithmetic is the one-launch iteration's: every output and statistic of objgrad,
    hprod Val(2) and solve_two_mixed BITWISE those of FPSQ_MULTI_ITER=1, over changing points (a first call has no expected
    count and runs one iteration per launch; from the second on the expected count is cut into launches of <= kmax)."""
    qp = _small_pde(seed=19, n=size[0], m=size[1]) if len(size) == 2 else problems.pde_control_like(n=size[0], m=size[1], seed=33)
    A = qp.scipy_csr()
    rng = np.random.default_rng(9)
    xs = [qp.xhat + 0.3 * 0.6 ** k * rng.standard_normal(qp.n) for k in range(4)]
    vs = [rng.standard_normal(qp.n) for _ in range(4)]

    def run(expect_multi):
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
        out, shared = [], 0
        for k, x in enumerate(xs):
            gx, ys, gs, hv = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.n)
            f, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs)
            i = dev.info()
            shared += i["last_multi_iterations"]
            assert i["last_multi_iterations"] <= i["last_fused_launches"] and i["last_multi_launches"] * kmax >= i["last_multi_iterations"]
            st = [(dev.stats[q].niter, dev.stats[q].status, dev.stats[q].rnorm, dev.stats[q].arnorm) for q in range(2)]
            rch = dev.hprod(vs[k], hv, 2)
            shared += dev.info()["last_multi_iterations"]
            o = [np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)]
            rcm = dev.solve_two_mixed(qp.qdiag * x + qp.d, A @ x - qp.b, *o)
            out += [np.array([f, rc, rch, rcm]), gx, ys, gs, hv, *o, np.array(st).ravel()]
        i = dev.info()
        assert i["wait_timeouts"] == 0 and i["fuse_fallbacks"] == 0
        dev.close()
        assert (shared > 0) == expect_multi, shared
        return out

    monkeypatch.setenv("FPSQ_FUSE_ITER", "2")
    monkeypatch.setenv("FPSQ_MULTI_ITER", "1")
    want = run(False)
    monkeypatch.setenv("FPSQ_MULTI_ITER", str(kmax))
    got = run(True)
    for i, (a_, b_) in enumerate(zip(got, want)):
        assert np.array_equal(a_, b_), i


@pytest.mark.parametrize("size,delta,eta", [((24000, 2400), 0.0, 2.0), ((60000, 6000), SE, 0.0),
                                            ((300000, 30000, "headline density"), 0.0, 0.0), ((300000, 30000, "headline density"), SE, 0.5)])
def test_one_launch_tail_is_bitwise_the_two_launch_tail(monkeypatch, size, delta, eta):
    """The tail of an evaluation on one GPU (round 5): the rows of the raw product A'[q1, c] go straight into grad(phi) -- k_spmv<.., GRAD>,
    csrc/fpsq_spmv.hip.h; its last workgroup reduces phi -- instead of being written, re-read and combined by k_qp_penalty_grad
    (FPSQ_FUSE_TAIL=0: those two launches).  One spelling of the row's arithmetic serves both (qp_grad_row): phi, gx, gs, ys, the
    statistics BITWISE the same, with and without the proximal term, one launch fewer per evaluation; the same for hprod! Val(2), whose
    single-lane product A'(A v) writes Hv as its row epilogue instead of handing J'Jv to k_qp_hprod_fin (qp_hfin_row); speculative (gated) tails included -- the points change so that the expected iteration count is wrong now and then."""
    qp = _small_pde(seed=23, n=size[0], m=size[1]) if len(size) == 2 else problems.pde_control_like(n=size[0], m=size[1], seed=35)
    rng = np.random.default_rng(13)
    xs = [qp.xhat + 0.5 ** (k % 5) * (1.0 if k % 3 else 1e-2) * rng.standard_normal(qp.n) for k in range(8)]
    xks = [qp.xhat + 0.1 * rng.standard_normal(qp.n) for _ in xs]
    vs = [rng.standard_normal(qp.n) for _ in xs]

    def run():
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta, eta=eta)
        out, launches = [], []
        for k, x in enumerate(xs):
            gx, ys, gs, hv = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.n)
            f, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xks[k] if eta > 0 else None)
            launches.append(dev.info()["last_kernel_launches"])
            st = [(dev.stats[q].niter, dev.stats[q].status, dev.stats[q].rnorm, dev.stats[q].arnorm) for q in range(2)]
            rch = dev.hprod(vs[k], hv, 2) if k % 2 else 0
            out += [np.array([f, rc, rch]), gx, ys, gs, hv if k % 2 else np.zeros(1), np.array(st).ravel()]
        dev.close()
        return out, launches

    monkeypatch.setenv("FPSQ_FUSE_TAIL", "0")
    want, l2 = run()
    monkeypatch.setenv("FPSQ_FUSE_TAIL", "1")
    got, l1 = run()
    for i, (a_, b_) in enumerate(zip(got, want)):
        assert np.array_equal(a_, b_), i
    # (one launch fewer per ENQUEUED tail: a speculative tail whose gates stay closed is enqueued again behind the loop)
    # (the first call has no expected count: how many look-ahead launches it enqueues depends on timing)
    assert all(a < b for a, b in zip(l1[1:], l2[1:])) and l1[-1] + 1 == l2[-1], (l1, l2)


def test_hprod_tail_on_a_replicated_communicator_of_one(monkeypatch):
    """hprod! Val(2) on a row-sharded handle of ONE shard without halo (replicated n-vectors: --parallel shard-allreduce at world 1).
    Its A'(A v) product needs no sum over the ranks, so the tail is the single-GPU one: k_spmv<1, .., GRAD> writes Hv as the row
    epilogue of the product.  FPSQ_FUSE_TAIL=0 (raw product, all-reduce, k_axpby_plain into J'Jv, k_qp_hprod_fin) gives Hv bitwise,
    with two kernel launches more; Hv matches a single-GPU handle's (the replicated loop forms its norms through other kernels)."""
    from fps_amd.device_qp import LocalGroup
    from fps_amd.distributed import shard_qp

    qp = _small_pde(seed=23, n=24000, m=2400)
    v = np.random.default_rng(5).standard_normal(qp.n)
    ref = DeviceEqQP(qp, sigma=1e3, rho=1.0)
    hv_ref = np.empty(qp.n)
    assert ref.hprod(v, hv_ref, 2) == 0
    ref.close()

    def run():
        group = LocalGroup(1)
        dev = DeviceEqQP(shard_qp(qp, 0, qp.m), sigma=1e3, rho=1.0, comm=("local", group.ptr, 0))
        hv = np.empty(qp.n)
        rc = group.run([lambda: dev.hprod(v, hv, 2)])[0]
        i = dev.info()
        st = [(dev.stats[q].niter, dev.stats[q].status) for q in range(2)]
        dev.close()
        group.close()
        assert rc == 0 and i["at_sorted"] != 0, i  # (the A' layout has a GRAD variant)
        return hv, st, i["last_kernel_launches"]

    monkeypatch.setenv("FPSQ_FUSE_TAIL", "0")
    hv2, st2, l2 = run()
    monkeypatch.setenv("FPSQ_FUSE_TAIL", "1")
    hv1, st1, l1 = run()
    assert np.array_equal(hv1, hv2) and st1 == st2
    assert l2 - l1 == 2, (l1, l2)
    assert _rel(hv1, hv_ref) < 1e-9


@pytest.mark.parametrize("size", [(24000, 2400), (300000, 30000, "headline density")])
def test_enqueueing_on_the_registered_stream_is_bitwise_the_own_stream(monkeypatch, size):
    """include/fpsq.h INPUT READINESS (round 5): with device-resident arguments whose producer stream is registered
    (fpsq_set_input_stream -- DeviceEqQP does that for torch tensors), a single-GPU handle enqueues ON that stream; FPSQ_ADOPT_STREAM=0
    keeps its own stream and orders with an event pair at both ends of a call.  Same kernels, same order: objgrad / hprod / the
    Jacobian refresh BITWISE the same -- on torch's default stream, on a side stream with work of the caller's queued in front
    (x is produced by a kernel of that stream: the evaluation must see the produced values) and after switching streams between
    calls; stream-ordered outputs are consumed on the same stream without a host synchronisation in between."""
    torch = pytest.importorskip("torch")
    qp = _small_pde(seed=27, n=size[0], m=size[1]) if len(size) == 2 else problems.pde_control_like(n=size[0], m=size[1], seed=37)
    dev0 = torch.device("cuda:0")
    rng = np.random.default_rng(17)
    xs_h = [qp.xhat + 0.5 ** (k % 4) * rng.standard_normal(qp.n) for k in range(6)]
    vs_h = [rng.standard_normal(qp.n) for _ in xs_h]

    def run():
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=SE)
        side = torch.cuda.Stream(device=dev0)
        out = []
        base = torch.from_numpy(np.stack(xs_h)).to(dev0)
        vs = torch.from_numpy(np.stack(vs_h)).to(dev0)
        vals = torch.from_numpy(np.ascontiguousarray(qp.vals)).to(dev0)
        torch.cuda.synchronize()
        for k in range(len(xs_h)):
            stream = torch.cuda.current_stream() if k < 2 else side if k < 5 else torch.cuda.current_stream()   # (two switches)
            with torch.cuda.stream(stream):
                x = base[k] * 2.0 - base[k]             # produced on `stream`, right in front of the call
                gx = torch.empty(qp.n, dtype=torch.float64, device=dev0)
                ys = torch.empty(qp.m, dtype=torch.float64, device=dev0)
                if k == 3:
                    dev.set_jacobian_values(vals * 1.0)  # (a refresh from a device array produced on the same stream)
                f, rc = dev.objgrad(x, gx=gx, ys=ys)
                chk = (gx * gx).sum()                    # consumed on the same stream, no host synchronisation in between
                hv = torch.empty(qp.n, dtype=torch.float64, device=dev0)
                rch = dev.hprod(vs[k], hv, 2) if k % 2 else 0
                st = [(dev.stats[q].niter, dev.stats[q].rnorm) for q in range(2)]
                stream.synchronize()
                out += [np.array([f, rc, rch, float(chk)]), gx.cpu().numpy(), ys.cpu().numpy(), hv.cpu().numpy() if k % 2 else np.zeros(1),
                        np.array(st).ravel()]
        i = dev.info()
        assert i["wait_timeouts"] == 0 and i["fuse_fallbacks"] == 0
        dev.close()
        return out

    monkeypatch.setenv("FPSQ_ADOPT_STREAM", "0")
    want = run()
    monkeypatch.setenv("FPSQ_ADOPT_STREAM", "1")
    got = run()
    for i, (a_, b_) in enumerate(zip(got, want)):
        assert np.array_equal(a_, b_), i
    # ... and the host-pointer path (nothing registered) agrees with both
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=SE)
    gx, ys = np.empty(qp.n), np.empty(qp.m)
    f, rc = dev.objgrad(xs_h[0], gx=gx, ys=ys)
    dev.close()
    assert f == got[0][0] and np.array_equal(gx, got[1]) and np.array_equal(ys, got[2])


@pytest.mark.parametrize("late", [0, 8, 3, 13])
def test_one_launch_iterations_with_a_late_mid_leader(monkeypatch, late):
    """The mid leaders of a fused launch publish per XCC, so the row groups of the other XCCs do not wait for a mid leader that
    another kernel holds up -- and when they reach their epilogues they WRITE the A product's norm partials, which that late
    leader, still redoing the head step, reads as the partials of the PREVIOUS A product.  The A partials therefore alternate
    between two arrays from launch to launch.  FPSQ_DEBUG_RIDE_DELAY_MID=c+1 holds mid leader c back by ~100 us (a committing
    one of either lane, two publishing-only ones): bitwise the two-launch iteration."""
    qp = problems.pde_control_like(n=300000, m=30000, seed=43)
    rng = np.random.default_rng(16)
    xs = [qp.xhat + 0.3 * 0.5 ** k * rng.standard_normal(qp.n) for k in range(3)]

    def run(expect_fused):
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
        out, fused = [], 0
        for x in xs:
            gx, ys, gs = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
            f, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs)
            fused += dev.info()["last_fused_launches"]
            out += [np.array([f, rc, dev.stats[0].niter, dev.stats[1].niter, dev.stats[0].rnorm, dev.stats[1].rnorm]), gx, ys, gs]
        dev.close()
        assert (fused > 0) == expect_fused
        return out

    monkeypatch.setenv("FPSQ_AT_ROW_ALIGN", "8")
    monkeypatch.setenv("FPSQ_FUSE_ITER", "0")
    want = run(False)
    monkeypatch.setenv("FPSQ_FUSE_ITER", "2")
    monkeypatch.setenv("FPSQ_DEBUG_RIDE_DELAY_MID", str(late + 1))
    got = run(True)
    for i, (a_, b_) in enumerate(zip(got, want)):
        assert np.array_equal(a_, b_), i


@pytest.mark.parametrize("rot", [1, 3, 4])
def test_one_launch_iterations_with_every_hand_over_across_xcds(monkeypatch, rot):
    """Both products of a fused launch walk XCD-contiguous eighths, so most rows a row group gathers were written on its own
    XCD, where one L2 makes the hand-over trivially coherent.  FPSQ_DEBUG_FUSE_ROTATE=r lets the A' workgroups of XCD x walk
    eighth (x + r) mod 8 instead: EVERY row a row group waits for has then been written through from another XCD, and the
    written-through stores + flags + agent-scope gathers carry the whole exchange.  Bitwise the two-launch iteration."""
    qp = problems.pde_control_like(n=300000, m=30000, seed=37)
    rng = np.random.default_rng(14)
    xs = [qp.xhat + 0.3 * 0.5 ** k * rng.standard_normal(qp.n) for k in range(4)]

    def run(expect_fused):
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
        out, fused = [], 0
        for x in xs:
            gx, ys, gs = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
            f, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs)
            fused += dev.info()["last_fused_launches"]
            out += [np.array([f, rc, dev.stats[0].niter, dev.stats[1].niter]), gx, ys, gs]
        dev.close()
        assert (fused > 0) == expect_fused
        return out

    monkeypatch.setenv("FPSQ_AT_ROW_ALIGN", "8")
    monkeypatch.setenv("FPSQ_FUSE_ITER", "0")
    want = run(False)
    monkeypatch.setenv("FPSQ_FUSE_ITER", "2")
    monkeypatch.setenv("FPSQ_DEBUG_FUSE_ROTATE", str(rot))
    got = run(True)
    for i, (a_, b_) in enumerate(zip(got, want)):
        assert np.array_equal(a_, b_), i


@pytest.mark.parametrize("late", [0, 8, 5])
@pytest.mark.parametrize("ln_method", [0, 1])
def test_one_launch_iterations_with_a_late_leader_and_lnlq(monkeypatch, late, ln_method):
    """The same with a head leader held back by ~100 us (a committing one of either lane, a publishing-only one) -- the mid
    leaders then finish the step behind the A' product while a head leader has not even read the state yet, which is why that
    step lands in a THIRD copy of the state -- and with LNLQ (ln_method = 1) as the least-norm recurrence."""
    qp = _small_pde(seed=23, n=60000, m=6000)
    rng = np.random.default_rng(9)
    xs = [qp.xhat + 0.3 * rng.standard_normal(qp.n) for _ in range(3)]

    def run(expect_fused):
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0, ln_method=ln_method)
        out, fused = [], 0
        for x in xs:
            gx, ys = np.empty(qp.n), np.empty(qp.m)
            f, rc = dev.objgrad(x, gx=gx, ys=ys)
            fused += dev.info()["last_fused_launches"]
            out += [np.array([f, rc, dev.stats[0].niter, dev.stats[1].niter, dev.stats[0].rnorm, dev.stats[1].rnorm]), gx, ys]
        dev.close()
        assert (fused > 0) == expect_fused
        return out

    monkeypatch.setenv("FPSQ_AT_ROW_ALIGN", "8")
    monkeypatch.setenv("FPSQ_FUSE_ITER", "0")
    want = run(False)
    monkeypatch.setenv("FPSQ_FUSE_ITER", "2")
    monkeypatch.setenv("FPSQ_DEBUG_RIDE_DELAY", str(late + 1))
    got = run(True)
    for i, (a_, b_) in enumerate(zip(got, want)):
        assert np.array_equal(a_, b_), i


@pytest.mark.parametrize("size", [(6000, 600), (300000, 30000)])
def test_minres_stages_in_one_launch_are_bitwise_the_three_launches(monkeypatch, size):
    """A MINRES lane (solve_two_extras, hprod! Val(1)) runs its stage E1, the scalar step A and stage E2 as ONE launch
    (k_minres_mid: every workgroup does E1 on its elements, publishes its partial as self-validating words, waits for the
    leader's record and does E2 on the same elements).  Same sums in the same order: every output and statistic of
    solve_two_extras and hprod Val(1) must be BITWISE those of a handle that launches the three separately
    (FPSQ_MINRES_MERGE=0), including a zero second right-hand side (the lane ends at once) and repeated calls."""
    qp = _small_pde(seed=41, n=size[0], m=size[1])
    A = qp.scipy_csr()
    rng = np.random.default_rng(15)
    r1s = [rng.standard_normal(qp.n) for _ in range(3)]
    r2s = [rng.standard_normal(qp.m), np.zeros(qp.m), rng.standard_normal(qp.m)]
    vs = [rng.standard_normal(qp.n) for _ in range(2)]

    def run():
        raw = _Handle(A, 0.0)
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
        out = []
        for r1, r2 in zip(r1s, r2s):
            e1, e2, rc = raw.solve_two_extras(r1, r2)
            st = [(raw.st[i].niter, raw.st[i].status, raw.st[i].rnorm, raw.st[i].arnorm) for i in range(2)]
            out += [e1, e2, np.array([rc]), np.array(st).ravel()]
        gx = np.empty(qp.n)
        dev.objgrad(qp.xhat + 0.2 * vs[0], gx=gx)
        for v in vs:
            hv = np.empty(qp.n)
            rch = dev.hprod(v, hv, 1)
            st = [(dev.stats4[i].niter, dev.stats4[i].status, dev.stats4[i].rnorm) for i in range(4)]
            out += [hv, np.array([rch]), np.array(st).ravel()]
        raw.close()
        dev.close()
        return out

    monkeypatch.setenv("FPSQ_MINRES_MERGE", "0")
    want = run()
    monkeypatch.setenv("FPSQ_MINRES_MERGE", "1")
    got = run()
    assert int(want[3][4]) > 2  # (the MINRES lane iterated)
    for i, (a_, b_) in enumerate(zip(got, want)):
        assert np.array_equal(a_, b_), i


def test_two_handles_iterating_at_once_with_one_launch_iterations(monkeypatch):
    """Two handles evaluating at the same time (two host threads, two streams): both grids are full of workgroups that wait for
    other workgroups of their own launch -- row groups for A' blocks, mid leaders for every block, updates for records -- and
    compete for the same XCDs.  Every dependence points to a workgroup EARLIER in its own grid, every XCD has its own leaders,
    and a waiting workgroup holds a quarter of a CU, not an XCD: the waits must end, and every result must equal the
    handle's own single-threaded one bitwise.  (Grids of several resident sets each: 1.3 resident sets of A' blocks + the row
    groups per handle.)"""
    import threading
    monkeypatch.setenv("FPSQ_FUSE_ITER", "2")
    qps = [_small_pde(seed=31, n=300000, m=30000), _small_pde(seed=32, n=260000, m=26000)]
    devs = [DeviceEqQP(q, sigma=1e3, rho=1.0, delta=0.0) for q in qps]
    rng = np.random.default_rng(12)
    xs = [[q.xhat + 0.3 * rng.standard_normal(q.n) for _ in range(3)] for q in qps]

    def evaluate(dev, q, x):
        gx, ys = np.empty(q.n), np.empty(q.m)
        f, rc = dev.objgrad(x, gx=gx, ys=ys)
        return [np.array([f, rc, dev.stats[0].niter, dev.stats[1].niter, dev.info()["last_fused_launches"] > 0]), gx, ys]

    want = [[evaluate(d, q, x) for x in xx] for d, q, xx in zip(devs, qps, xs)]
    assert all(w[0][4] for ww in want for w in ww)
    bad = []

    def work(k):
        try:
            for rep in range(12):
                for x, w in zip(xs[k], want[k]):
                    got = evaluate(devs[k], qps[k], x)
                    if not all(np.array_equal(a, b) for a, b in zip(got, w)):
                        bad.append(f"mismatch handle {k} rep {rep}")
        except BaseException as e:  # noqa: BLE001  (an assertion in a thread would otherwise vanish)
            bad.append(repr(e))

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad, bad[:3]
    for d in devs:
        d.close()


@pytest.mark.expects_wait_timeouts
def test_one_launch_iteration_bounded_waits_end_and_the_call_is_repeated_on_two_launches(monkeypatch, capfd):
    """Every wait of the fused launch has an end each wave reaches: with the A' blocks made to publish a wrong launch number
    (FPSQ_DEBUG_FUSE_BREAK=1) the row groups give up on their flags and the mid leaders on the tagged partials after their
    bounded numbers of looks, whoever waits for the mid leaders' record after its own; the handle's error word is raised,
    every kernel of the call ends, the handle switches to two launches per iteration and the entry point REPEATS the call --
    what a process sharing its GPU with others would see when their waiting workgroups starve its own (a delay, the right
    answer -- bitwise a two-launch handle's --, fpsq_info.fuse_fallbacks = wait_timeouts = 1, and with FPSQ_VERBOSE=1 one
    line on stderr).  Within seconds."""
    import time
    qp = _small_pde(seed=5, n=60000, m=6000)
    monkeypatch.setenv("FPSQ_AT_ROW_ALIGN", "8")
    monkeypatch.setenv("FPSQ_FUSE_ITER", "0")
    ref = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
    gx0 = np.empty(qp.n)
    f0, rc0 = ref.objgrad(qp.x, gx=gx0)
    ref.close()
    monkeypatch.setenv("FPSQ_FUSE_ITER", "2")
    monkeypatch.setenv("FPSQ_DEBUG_FUSE_BREAK", "1")
    monkeypatch.setenv("FPSQ_VERBOSE", "1")
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
    gx = np.empty(qp.n)
    t0 = time.perf_counter()
    f, rc = dev.objgrad(qp.x, gx=gx)
    assert time.perf_counter() - t0 < 60.0
    i = dev.info()
    assert rc == rc0 and f == f0 and np.array_equal(gx, gx0) and i["last_fused_launches"] == 0
    assert i["fuse_fallbacks"] == 1 and i["wait_timeouts"] == 1 and i["p2p_timeouts"] == 0
    assert "bounded wait of a one-launch iteration expired" in capfd.readouterr().err
    f, rc = dev.objgrad(qp.x, gx=gx)  # (and stays there)
    i = dev.info()
    assert np.array_equal(gx, gx0) and i["last_fused_launches"] == 0 and i["fuse_fallbacks"] == 1 and i["wait_timeouts"] == 1
    dev.close()
    monkeypatch.setenv("FPSQ_DEBUG_FUSE_BREAK", "0")
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
    gx2 = np.empty(qp.n)
    f2, rc = dev.objgrad(qp.x, gx=gx2)
    assert rc == 0 and np.array_equal(gx2, gx0) and dev.info()["last_fused_launches"] > 0
    dev.close()


@pytest.mark.expects_wait_timeouts
def test_riding_leaders_bounded_wait_ends_in_an_error_not_a_hang(monkeypatch):
    """Every wait of the leader protocol has an end each wave reaches: with the leaders made to publish a wrong launch number
    (FPSQ_DEBUG_RIDE_BREAK=1) the workgroups of the product give up after their bounded number of looks, raise the handle's
    error word and leave; the call returns FPSQ_ERR_TIMEOUT (-5) with a message, within seconds.  A fresh handle without
    the switch works as ever."""
    import time
    qp = _small_pde(seed=5, n=4000, m=400)
    monkeypatch.setenv("FPSQ_DEBUG_RIDE_BREAK", "1")
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0, ls_itmax=3, ln_itmax=3)
    gx = np.empty(qp.n)
    t0 = time.perf_counter()
    with pytest.raises(Exception) as ei:
        dev.objgrad(qp.x, gx=gx)
    assert time.perf_counter() - t0 < 30.0
    assert "bounded wait" in str(ei.value)
    dev.close()
    monkeypatch.setenv("FPSQ_DEBUG_RIDE_BREAK", "0")
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
    f, rc = dev.objgrad(qp.x, gx=gx)
    assert rc == 0 and np.all(np.isfinite(gx))
    dev.close()


def test_repeated_hprod_and_objgrad_calls_are_bitwise_identical():
    """The same call repeated on fresh and on warm handles gives the same bits every time (all reductions run in fixed
    orders; no atomics).  Regression test of the round-2 / round-3 race: the progress word used to be two stores, and a host
    that caught `iter` without `done` applied the final LSQR update twice (~1e-6 in Hv, 2-8 % of the calls of this loop)."""
    qp = _small_pde(seed=31, n=3000, m=300)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(qp.n)
    x = qp.xhat + 0.2 * rng.standard_normal(qp.n)
    want = None
    for rep in range(12):
        dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
        for call in range(4):
            hv, gx, ys = np.empty(qp.n), np.empty(qp.n), np.empty(qp.m)
            assert dev.hprod(v, hv, 1 + call % 2) == 0
            f, rc = dev.objgrad(x, gx=gx, ys=ys)
            got = (hv, gx, ys, np.array([f]))
            if want is None:
                want = [a.copy() for a in got]
            for a, b in zip(got, want):
                assert np.array_equal(a, b), (rep, call)
        dev.close()


# ---------------------------------------------------------------------------------------------- row sharding

@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("delta", [0.0, SE])
def test_row_sharded_objgrad_matches_single_gpu(oracle, nshards, delta):
    """The sharded code path (raw partial A' products -> all-reduce -> fused axpby + norm; scalar all-reduce of the
    m-vector sums) with the in-process loopback communicator: same iteration counts and the same grad(phi) as the
    unsharded handle (only the summation order of the reductions differs: 1e-9)."""
    from fps_amd.device_qp import LocalGroup
    from fps_amd.distributed import row_partition, shard_qp

    qp = _small_pde(seed=21, n=4000, m=400)
    ref = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=delta)
    g_ref, ys_ref = np.empty(qp.n), np.empty(qp.m)
    f_ref, rc_ref = ref.objgrad(qp.x, gx=g_ref, ys=ys_ref)
    it_ref = (ref.stats[0].niter, ref.stats[1].niter)
    ref.close()

    bounds = row_partition(qp.rowptr, nshards)
    assert bounds[0] == 0 and bounds[-1] == qp.m and np.all(np.diff(bounds) > 0)
    group = LocalGroup(nshards)
    shards = [DeviceEqQP(shard_qp(qp, bounds[r], bounds[r + 1]), sigma=1e3, rho=1.0, delta=delta,
                         comm=("local", group.ptr, r)) for r in range(nshards)]
    gs = [np.empty(qp.n) for _ in range(nshards)]
    yss = [np.empty(bounds[r + 1] - bounds[r]) for r in range(nshards)]
    res = group.run([lambda r=r: shards[r].objgrad(qp.x, gx=gs[r], ys=yss[r]) for r in range(nshards)])
    for r in range(nshards):
        f, rc = res[r]
        assert rc == rc_ref == 0
        assert (shards[r].stats[0].niter, shards[r].stats[1].niter) == it_ref
        assert abs(f - f_ref) <= 1e-9 * abs(f_ref)
        assert _rel(gs[r], g_ref) < 1e-9
        assert np.array_equal(gs[r], gs[0]), "replicated n-vectors must be bitwise identical on every shard"
    assert _rel(np.concatenate(yss), ys_ref) < 1e-9
    for sh in shards:
        sh.close()
    group.close()


@pytest.mark.parametrize("nshards,p2p", [(2, False), (3, False), (8, False), (2, True), (3, True), (2, "in-launch"), (3, "in-launch"),
                                         (2, "in-launch-fused"), (3, "in-launch-fused")])
@pytest.mark.parametrize("delta", [0.0, SE])
def test_halo_sharded_objgrad_hprod_match_single_gpu(oracle, nshards, p2p, delta, monkeypatch):
    """HALO mode (include/fpsq.h fpsq_comm_set_halo; the SURVEY 8e contract path): every shard holds only its column
    window of the n-vectors and exchanges the partial A'u products of its two overlap regions with its neighbours
    (in-process communicator: copy kernels instead of ncclSend/ncclRecv) plus 4-double all-reduces.  objgrad and hprod
    on 2 / 3 / 8 shards reproduce the unsharded handle (iteration counts identical, values to 1e-9: only the order of
    the reductions differs); overlaps are bitwise identical on the two ranks that share them; phi is bitwise
    identical on all shards (replicated scalars).  p2p: the same through the PEER-TO-PEER route (fpsq_local_group_set_p2p:
    halo records and norm partials written straight into the peers' buffers, sequence flags, bounded waits -- the protocol
    of the xGMI route, no collective call in the loop).  "in-launch" (round 5; FPSQ_LX=2 forces it between shards of one device,
    whose small grids are resident all at once): the sums over the ranks are formed INSIDE the launches that need them -- the
    leader workgroups and the phi reduction write their local sums into the peers' receive areas and add the rows up in rank
    order (fpsq_krylov.hip.h xch_sum): no gather kernel; fpsq_info.comm_in_launch_sums = 1.  "in-launch-fused": additionally
    ONE launch per joint iteration on every shard (FPSQ_FUSE_ITER=2: wherever possible) -- the exchange and the finish of the
    overlap rows ride in it too (k_iter_fused<.., HALO>, fuse_halo_wg)."""
    from fps_amd.device_qp import LocalGroup
    from fps_amd.distributed import halo_plan, row_partition, shard_qp_halo

    fused = p2p == "in-launch-fused"
    in_launch = p2p in ("in-launch", "in-launch-fused")
    if in_launch:
        monkeypatch.setenv("FPSQ_LX", "2")
        monkeypatch.setenv("FPSQ_FUSE_ITER", "2" if fused else "0")
        p2p = True
    qp = problems.pde_control_like(n=24000, m=2400, per_row=24, window=512, seed=29)
    sigma, rho = 1e3, 1.0
    ref = DeviceEqQP(qp, sigma=sigma, rho=rho, delta=delta)
    g_ref, ys_ref, gs_ref = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
    f_ref, rc_ref = ref.objgrad(qp.x, gx=g_ref, ys=ys_ref, gs=gs_ref)
    it_ref = (ref.stats[0].niter, ref.stats[1].niter)
    v = np.random.default_rng(3).standard_normal(qp.n)
    hv_ref = np.empty(qp.n)
    assert ref.hprod(v, hv_ref) == 0
    ith_ref = (ref.stats[0].niter, ref.stats[1].niter)
    ref.close()

    bounds = row_partition(qp.rowptr, nshards)
    plan = halo_plan(qp.rowptr, qp.colind, qp.n, bounds)
    assert plan is not None and plan.max_exchange_doubles() <= 2 * 2 * 512
    group = LocalGroup(nshards, p2p=p2p)
    locs = [shard_qp_halo(qp, plan, r) for r in range(nshards)]
    shards = [DeviceEqQP(locs[r], sigma=sigma, rho=rho, delta=delta, comm=("local", group.ptr, r),
                         halo=plan.overlaps(r)) for r in range(nshards)]
    gx = [np.empty(l.n) for l in locs]
    gs = [np.empty(l.n) for l in locs]
    ys = [np.empty(l.m) for l in locs]
    res = group.run([lambda r=r: shards[r].objgrad(locs[r].x, gx=gx[r], ys=ys[r], gs=gs[r]) for r in range(nshards)])
    for r in range(nshards):
        f, rc = res[r]
        assert rc == rc_ref == 0
        assert (shards[r].stats[0].niter, shards[r].stats[1].niter) == it_ref
        assert f == res[0][0] and abs(f - f_ref) <= 1e-9 * abs(f_ref)
        i = shards[r].info()
        assert i["comm_in_launch_sums"] == (1 if in_launch else 0) and i["p2p_timeouts"] == 0
        if fused:      # per joint iteration: ONE launch (+ the stand-alone step in front of the gated epilogue)
            # (a first call has no expected count: every `lookahead` = 4 iterations a stand-alone step shows the host where it is,
            # and the iteration behind it runs on separate launches)
            assert i["last_fused_launches"] >= i["last_loop_iterations"] - i["last_loop_iterations"] // 4 - 1 > 0, i
            assert i["last_loop_launches"] <= i["last_loop_iterations"] + 3 * (i["last_loop_iterations"] // 4) + 3, i
        elif in_launch:  # per joint iteration: the two product launches + the halo launch, no gather kernel
            assert i["last_loop_launches"] <= 3 * i["last_loop_iterations"] + i["last_loop_iterations"] // 4 + 3, i
        if r + 1 < nshards:  # the overlap with the right neighbour: same global columns, bitwise equal
            t = plan.overlaps(r)[1]
            assert t > 0 and np.array_equal(gx[r][-t:], gx[r + 1][:t]) and np.array_equal(gs[r][-t:], gs[r + 1][:t])
    assert _rel(plan.assemble(gx), g_ref) < 1e-9 and _rel(plan.assemble(gs), gs_ref) < 1e-9
    assert _rel(np.concatenate(ys), ys_ref) < 1e-9
    # hprod! Val(2) on the sharded handles (two LSQR lanes + rho A'(A v))
    hv = [np.empty(l.n) for l in locs]
    rcs = group.run([lambda r=r: shards[r].hprod(v[plan.window(r)], hv[r]) for r in range(nshards)])
    assert all(rc == 0 for rc in rcs)
    assert all((sh.stats[0].niter, sh.stats[1].niter) == ith_ref for sh in shards)
    assert _rel(plan.assemble(hv), hv_ref) < 1e-9
    # ... and Val(1) (adds the LSQR + MINRES lanes of solve_two_extras): the same product on this model
    hv1 = [np.empty(l.n) for l in locs]
    rcs = group.run([lambda r=r: shards[r].hprod(v[plan.window(r)], hv1[r], 1) for r in range(nshards)])
    assert all(rc == 0 for rc in rcs) and all(np.array_equal(a, b) for a, b in zip(hv, hv1))
    assert all(sh.stats4[3].status == 1 for sh in shards)  # MINRES, zero right-hand side
    # the seam itself: solve_two_mixed / solve_two_least_squares with window right-hand sides
    A = qp.scipy_csr()
    g = qp.qdiag * qp.x + qp.d
    c = A @ qp.x - qp.b
    outs = [[np.empty(l.n), np.empty(l.m), np.empty(l.n), np.empty(l.m)] for l in locs]
    group.run([lambda r=r: shards[r].solve_two_mixed(g[plan.window(r)], c[bounds[r]:bounds[r + 1]], *outs[r])
               for r in range(nshards)])
    o = oracle.solve_two_mixed(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, g, c)
    assert all((sh.stats[0].niter, sh.stats[1].niter) == (o[4][0].niter, o[4][1].niter) for sh in shards)
    assert _rel(plan.assemble([x[0] for x in outs]), o[0]) < 1e-8 and _rel(np.concatenate([x[1] for x in outs]), o[1]) < 1e-8
    assert _rel(plan.assemble([x[2] for x in outs]), o[2]) < 1e-8 and _rel(np.concatenate([x[3] for x in outs]), o[3]) < 1e-8
    # solve_two_extras (LSQR + MINRES lanes) on the sharded handles
    r2 = np.random.default_rng(4).standard_normal(qp.m)
    ex = [[np.empty(l.m), np.empty(l.m)] for l in locs]
    lib = shards[0]._lib

    def extras(r):
        sh = shards[r]
        gw = np.ascontiguousarray(g[plan.window(r)])
        rw = np.ascontiguousarray(r2[bounds[r]:bounds[r + 1]])
        return sh._check(lib.fpsq_solve_two_extras(sh._h, gw.ctypes.data, rw.ctypes.data, ex[r][0].ctypes.data,
                                                   ex[r][1].ctypes.data, sh.stats))

    group.run([lambda r=r: extras(r) for r in range(nshards)])
    oe = oracle.solve_two_extras(qp.m, qp.n, qp.rowptr, qp.colind, qp.vals, delta, g, r2)
    assert all((sh.stats[0].niter, sh.stats[1].niter) == (oe[2][0].niter, oe[2][1].niter) for sh in shards)
    assert _rel(np.concatenate([x[0] for x in ex]), oe[0]) < 1e-8 and _rel(np.concatenate([x[1] for x in ex]), oe[1]) < 1e-8
    for sh in shards:
        sh.close()
    group.close()


@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("delta", [0.0, SE])
def test_sharded_one_launch_iterations_are_bitwise_the_three_launch_iterations(nshards, delta, monkeypatch):
    """A halo-sharded handle with rows shared with its neighbours: ONE launch per joint iteration (A' product, the push of the raw
    overlap sums into the neighbours' slots, the finish of the overlap rows, both steps with their sums over the ranks, the A
    product -- k_iter_fused<.., HALO>) against the same handle on three launches per iteration (A' product, k_p2p_halo_finish, A
    product; FPSQ_FUSE_ITER=0): same per-block, per-row and per-rank arithmetic, the partials summed in the same order --
    BITWISE equal gradients, multipliers, Hessian products, phi and statistics, over changing points."""
    from fps_amd.device_qp import LocalGroup
    from fps_amd.distributed import halo_plan, row_partition, shard_qp_halo

    qp = problems.pde_control_like(n=24000, m=2400, per_row=24, window=512, seed=31)
    bounds = row_partition(qp.rowptr, nshards)
    plan = halo_plan(qp.rowptr, qp.colind, qp.n, bounds)
    assert plan is not None
    locs = [shard_qp_halo(qp, plan, r) for r in range(nshards)]
    for r in range(nshards):
        left, right = plan.overlaps(r)
        assert left % 8 == 0 and (locs[r].n - right) % 8 == 0 and left + right > 0   # (halo_plan: regions on 128-byte lines)
    monkeypatch.setenv("FPSQ_LX", "2")
    monkeypatch.setenv("FPSQ_AT_ROW_ALIGN", "8")   # (the block boundaries of the one-launch layout for both handles: same partial sums)
    v = np.random.default_rng(5).standard_normal(qp.n)
    got = {}
    for mode in ("0", "2"):
        monkeypatch.setenv("FPSQ_FUSE_ITER", mode)
        group = LocalGroup(nshards, p2p=True)
        shards = [DeviceEqQP(locs[r], sigma=1e3, rho=1.0, delta=delta, comm=("local", group.ptr, r), halo=plan.overlaps(r))
                  for r in range(nshards)]
        rec = []
        for k in range(4):
            xk = qp.point(1 + k)
            gx = [np.empty(l.n) for l in locs]
            ys = [np.empty(l.m) for l in locs]
            res = group.run([lambda r=r: shards[r].objgrad(np.ascontiguousarray(xk[plan.window(r)]), gx=gx[r], ys=ys[r])
                             for r in range(nshards)])
            rec.append((res, gx, ys, [(s_.stats[0].niter, s_.stats[1].niter, s_.stats[0].rnorm, s_.stats[1].rnorm) for s_ in shards]))
        hv = [np.empty(l.n) for l in locs]
        rcs = group.run([lambda r=r: shards[r].hprod(np.ascontiguousarray(v[plan.window(r)]), hv[r]) for r in range(nshards)])
        rec.append((rcs, hv, [(s_.stats[0].niter, s_.stats[1].niter) for s_ in shards]))
        infos = [s_.info() for s_ in shards]
        for i in infos:
            assert i["comm_in_launch_sums"] == 1 and i["p2p_timeouts"] == 0 and i["wait_timeouts"] == 0
            assert (i["last_fused_launches"] > 0) == (mode == "2"), i
        got[mode] = rec
        for s_ in shards:
            s_.close()
        group.close()
    a, b = got["0"], got["2"]
    for k in range(4):
        assert a[k][0] == b[k][0] and a[k][3] == b[k][3]
        for r in range(nshards):
            assert np.array_equal(a[k][1][r], b[k][1][r]) and np.array_equal(a[k][2][r], b[k][2][r])
    assert a[4][0] == b[4][0] and a[4][2] == b[4][2]
    for r in range(nshards):
        assert np.array_equal(a[4][1][r], b[4][1][r])


@pytest.mark.parametrize("extra", [1, 2])
def test_a_slow_reader_of_the_halo_slots_is_waited_for(monkeypatch, extra):
    """The wait of k_p2p_halo_finish for the neighbours comes first and is unconditional -- also in a launch with nothing to finish
    (the recurrences have ended, a gate is closed): it is what keeps a rank's next push of the same parity out of a slot a
    slower neighbour is still reading when no sum over the ranks lies between the two pushes (advisor / verdict, round 4).
    Set up here: two shards, sums over the ranks inside the launches (no gather kernel paces the ranks), three launches per
    iteration; shard 1 READS its halo slots ~100 us late in every launch (FPSQ_DEBUG_P2P_DELAY=2); the second evaluation is
    told to expect `extra` iterations more than it needs (fpsq_debug_expect_iterations): shard 0 runs launches with nothing to
    finish, then the epilogue's product, whose push goes into a slot shard 1 used shortly before.  Bitwise the first evaluation
    on both shards.  (A deterministic FAILING interleaving for the first build's early exit could not be constructed: in every
    launch sequence the host issues today a data-carrying exchange is followed by a sum over the ranks -- which needs the
    slow shard's finish workgroups -- before the next push of the same parity; an attempt with a debug switch that restored the
    early exit passed this very test.  The unconditional wait makes the slots safe by themselves, whatever the host enqueues.)"""
    from fps_amd.device_qp import LocalGroup
    from fps_amd.distributed import halo_plan, row_partition, shard_qp_halo

    qp = problems.pde_control_like(n=24000, m=2400, per_row=24, window=512, seed=37)
    plan = halo_plan(qp.rowptr, qp.colind, qp.n, row_partition(qp.rowptr, 2))
    locs = [shard_qp_halo(qp, plan, r) for r in range(2)]
    for k, v in (("FPSQ_LX", "2"), ("FPSQ_FUSE_ITER", "0"), ("FPSQ_DEBUG_P2P_DELAY", "2")):
        monkeypatch.setenv(k, v)
    group = LocalGroup(2, p2p=True)
    shards = [DeviceEqQP(locs[r], sigma=1e3, rho=1.0, delta=0.0, comm=("local", group.ptr, r), halo=plan.overlaps(r)) for r in range(2)]
    out = []
    for rep in range(2):
        gx = [np.empty(l.n) for l in locs]
        res = group.run([lambda r=r: shards[r].objgrad(locs[r].x, gx=gx[r]) for r in range(2)])
        its = [(s_.stats[0].niter, s_.stats[1].niter) for s_ in shards]
        out.append((res, gx, its))
        for s_ in shards:
            assert s_._lib.fpsq_debug_expect_iterations(s_._h, max(its[0]) + extra) == 0
    (r0, g0, i0), (r1, g1, i1) = out
    assert r0 == r1 and i0 == i1 and r0[0] == r0[1] and all(np.array_equal(a, b) for a, b in zip(g0, g1))
    for s_ in shards:
        assert s_.info()["p2p_timeouts"] == 0
        s_.close()
    group.close()


def test_halo_mode_argument_checks():
    """fpsq_comm_set_halo: needs a communicator; overlaps must fit the window and vanish at the outer ends."""
    from fps_amd.device_qp import LocalGroup
    from fps_amd.qdsolver import FpsqError

    qp = _small_pde(seed=23, n=3000, m=300)
    single = DeviceEqQP(qp)
    assert single._lib.fpsq_comm_set_halo(single._h, 0, 0) == -1  # no communicator
    single.close()
    group = LocalGroup(2)
    with pytest.raises(FpsqError):
        DeviceEqQP(qp, comm=("local", group.ptr, 0), halo=(5, 0))   # rank 0 has no left neighbour
    with pytest.raises(FpsqError):
        DeviceEqQP(qp, comm=("local", group.ptr, 1), halo=(2000, 2000))  # overlaps larger than the window
    ok = DeviceEqQP(qp, comm=("local", group.ptr, 1), halo=(100, 0))
    ok.close()
    group.close()


def test_rccl_single_rank_communicator():
    """world_size = 1 through the real RCCL path (the only RCCL configuration a one-GPU box can run)."""
    from fps_amd.device_qp import rccl_unique_id

    qp = _small_pde(seed=23, n=3000, m=300)
    a = DeviceEqQP(qp, delta=SE)
    b = DeviceEqQP(qp, delta=SE, comm=("rccl", 1, 0, rccl_unique_id()))
    ga, gb = np.empty(qp.n), np.empty(qp.n)
    fa, _ = a.objgrad(qp.x, gx=ga)
    fb, _ = b.objgrad(qp.x, gx=gb)
    assert (a.stats[0].niter, a.stats[1].niter) == (b.stats[0].niter, b.stats[1].niter)
    assert _rel(gb, ga) < 1e-9 and abs(fa - fb) <= 1e-9 * abs(fa)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- BASELINE configs

def test_config_aug2dc_like_full_size(oracle):
    """BASELINE configs[3] stand-in (AUG2DC-like, N = 100: n = 20200, m = 10000; NOT SIF-verified, parity unpinned
    against CUTEst): hundreds of Krylov iterations on an ill-conditioned incidence matrix; same iteration counts as
    the C restatement, grad(phi) equal to 1e-7 (rounding differences accumulate over ~10^3 iterations)."""
    qp = problems.aug2dc_like(N=100)
    assert (qp.n, qp.m) == (20200, 10000)
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=SE)
    gx, ys = np.empty(qp.n), np.empty(qp.m)
    fx, rc = dev.objgrad(qp.x, gx=gx, ys=ys)
    o = oracle.qp_objgrad(qp, qp.x, 1e3, 1.0, SE)
    assert rc == o["rc"]
    its = (dev.stats[0].niter, dev.stats[1].niter)
    its_o = (o["stats"][0].niter, o["stats"][1].niter)
    assert abs(its[0] - its_o[0]) <= 2 and abs(its[1] - its_o[1]) <= 2 and its[0] > 50
    assert _rel(gx, o["gx"]) < 1e-6 and _rel(ys, o["ys"]) < 1e-6
    dev.close()


def test_config_random_eqqp_cfg2_size(oracle):
    """BASELINE configs[1]: random sparse eq-QP n = 1e5, m = 1e4, nnz = 1e6 (columns spread over all of n)."""
    qp = problems.random_eqqp()
    assert (qp.n, qp.m, qp.nnz) == (100_000, 10_000, 1_000_000)
    dev = DeviceEqQP(qp, sigma=1e3, rho=1.0, delta=0.0)
    gx = np.empty(qp.n)
    fx, rc = dev.objgrad(qp.x, gx=gx)
    o = oracle.qp_objgrad(qp, qp.x, 1e3, 1.0, 0.0)
    assert rc == o["rc"] == 0
    assert (dev.stats[0].niter, dev.stats[1].niter) == (o["stats"][0].niter, o["stats"][1].niter)
    assert _rel(gx, o["gx"]) < 1e-8 and abs(fx - o["fx"]) <= 1e-8 * abs(o["fx"])
    dev.close()


@pytest.mark.parametrize("gen", ["stratified", "hashed"])
def test_config_headline_full_size_matches_oracle(oracle, gen):
    """(gen = hashed: the same shape with SURVEY 8(d)'s LITERAL column rule -- distinct hashed offsets in the 8192-column
    window, re-drawn on collision, problems.pde_control_hashed -- next to the stratified columns of the bench headline: the
    layouts must not live off the generator's regularity, and the parity bar is the same.)
    BASELINE configs[4] / the bench workload (n = 1e6, m = 1e5, nnz = 1e7) against the C restatement of the
    reference's iterative path at FULL size (one evaluation takes the single-threaded oracle ~0.5 s): identical
    iteration counts, status and `solved` flags of both Krylov recurrences, ys / gs / grad(phi) / phi to 1e-8 (same
    algorithm and tolerances; the differences are summation-order rounding amplified by sigma = 1e3).  delta = sqrt(eps)
    is the reference's delta_0 (parameters.jl:77): CRAIG then stops on ln_conlim (status ILL_COND, solved = false) in
    both implementations -- whether Krylov.jl does the same is what tests/golden/make_krylov_golden.jl can settle."""
    qp = (problems.pde_control_like if gen == "stratified" else problems.pde_control_hashed)(n=1_000_000, m=100_000)
    sigma, rho = 1e3, 1.0
    for delta in (0.0, SE):
        dev = DeviceEqQP(qp, sigma=sigma, rho=rho, delta=delta)
        for t in (3, 4):
            x = qp.point(t)
            gx, ys, gs = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
            fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs)
            o = oracle.qp_objgrad(qp, x, sigma, rho, delta)
            assert rc == o["rc"] == (0 if delta == 0.0 else 2)
            for k in range(2):
                got, want = dev.stats[k], o["stats"][k]
                assert (got.niter, got.status, got.solved, got.inconsistent) == \
                       (want.niter, want.status, want.solved, want.inconsistent)
                assert abs(got.rnorm - want.rnorm) <= 1e-6 * max(want.rnorm, 1e-300)
            assert dev.stats[0].niter > 10 and dev.stats[1].niter > 10  # Krylov really iterates here
            assert _rel(ys, o["ys"]) < 1e-8 and _rel(gs, o["gs"]) < 1e-8 and _rel(gx, o["gx"]) < 1e-8
            assert abs(fx - o["fx"]) <= 1e-8 * abs(o["fx"])
        # hprod! Val(2) at full size against the restatement of model:521-570
        v = qp.point(21) - qp.xhat
        Hv = np.empty(qp.n)
        rc = dev.hprod(v, Hv)
        oh = oracle.qp_hprod(qp, v, sigma, rho, delta)
        assert rc == oh["rc"] == 0
        assert (dev.stats[0].niter, dev.stats[1].niter) == (oh["stats"][0].niter, oh["stats"][1].niter)
        assert _rel(Hv, oh["Hv"]) < 1e-8
        # hprod! Val(1) (model:572-634) at full size: + the two recurrences of solve_two_extras
        Hv1 = np.empty(qp.n)
        rc = dev.hprod(v, Hv1, 1)
        o1 = oracle.qp_hprod(qp, v, sigma, rho, delta, approx=1)
        assert rc == o1["rc"]
        for k in range(4):
            assert (dev.stats4[k].niter, dev.stats4[k].status, dev.stats4[k].solved) == \
                   (o1["stats"][k].niter, o1["stats"][k].status, o1["stats"][k].solved), k
        assert _rel(Hv1, o1["Hv"]) < 1e-8
        dev.close()


def test_config_headline_full_size_properties():
    """BASELINE configs[4] / the bench workload (n = 1e6, m = 1e5, nnz = 1e7): size-independent properties checked with
    an independent host CSR (next to the direct comparison with the CPU restatement above): the KKT residuals of what
    the solves return, the closed forms of phi and grad(phi), and linearity of the solves."""
    import scipy.sparse as sp

    qp = problems.pde_control_like(n=1_000_000, m=100_000)
    assert (qp.n, qp.m) == (1_000_000, 100_000) and qp.nnz >= 10_000_000
    A = sp.csr_matrix((qp.vals, qp.colind, qp.rowptr), shape=(qp.m, qp.n))
    sigma, rho = 1e3, 1.0
    for delta in (0.0, SE):
        dev = DeviceEqQP(qp, sigma=sigma, rho=rho, delta=delta)
        x = qp.point(3)
        g = qp.qdiag * x + qp.d
        c = A @ x - qp.b
        # (1) the two systems of solve_two_mixed: K [p1; q1] = [g; 0],  K [p2; q2] = [0; c]
        p1, q1, p2, q2 = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)
        rc_mixed = dev.solve_two_mixed(g, c, p1, q1, p2, q2)
        # delta = sqrt(eps): CRAIG with M = (1/delta) I reaches the condition-number limit ln_conlim = 1/sqrt(eps) of
        # the reference's defaults (struct.jl:107) after 12 iterations and stops "ill-conditioned": a soft failure the
        # reference only warns about (linear_system.jl:136-138); the C restatement stops at the same iteration
        assert rc_mixed == (0 if delta == 0.0 else 2)
        it_mixed = (dev.stats[0].niter, dev.stats[1].niter)
        assert 5 <= it_mixed[0] <= 60 and 5 <= it_mixed[1] <= 60
        tol = 2e-6  # Krylov stop at sqrt(eps) relative residual estimates; cond(A) ~ 10 on this generator
        assert np.linalg.norm(p1 + A.T @ q1 - g) <= tol * np.linalg.norm(g)
        assert np.linalg.norm(A @ p1 - delta * q1) <= tol * np.linalg.norm(g)
        tol2 = tol if rc_mixed == 0 else 1e-3  # (the early "ill-conditioned" stop leaves a 1e-4 relative residual)
        assert np.linalg.norm(p2 + A.T @ q2) <= tol2 * np.linalg.norm(c)
        assert np.linalg.norm(A @ p2 - delta * q2 - c) <= tol2 * np.linalg.norm(c)
        # (2) objgrad closed forms from (ys, gs, v = p2):  model:244-248, 362-369, 385-397, 424-431
        gx, ys, gs = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
        fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs)
        assert rc == rc_mixed and (dev.stats[0].niter, dev.stats[1].niter) == it_mixed
        assert _rel(ys, q1 + sigma * q2) < 1e-12 and _rel(gs, p1 + sigma * p2) < 1e-12
        f = 0.5 * np.dot(x, qp.qdiag * x) + np.dot(qp.d, x)
        assert abs(fx - (f - np.dot(c, ys) + 0.5 * rho * np.dot(c, c))) <= 1e-11 * max(1.0, abs(fx))
        expect = gs - qp.qdiag * p2 + sigma * p2 + rho * (A.T @ c)
        assert _rel(gx, expect) < 1e-11
        # (3) solve_two_least_squares (hprod!): K [p; q] = [rhs; 0] for two right-hand sides at once; linear in rhs
        r1, r2 = qp.point(11), qp.point(12)
        a1, b1, a2, b2 = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)
        assert dev.solve_two_least_squares(r1, r2, a1, b1, a2, b2) == 0
        for rhs, pp, qq in ((r1, a1, b1), (r2, a2, b2)):
            assert np.linalg.norm(pp + A.T @ qq - rhs) <= tol * np.linalg.norm(rhs)
            assert np.linalg.norm(A @ pp - delta * qq) <= tol * np.linalg.norm(rhs)
        s1, t1, s2, t2 = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)
        assert dev.solve_two_least_squares(r1 + 2.0 * r2, r2, s1, t1, s2, t2) == 0
        assert _rel(t1, b1 + 2.0 * b2) < 1e-5 and _rel(t2, b2) < 1e-9
        dev.close()


def test_error_codes_of_the_c_abi():
    """Hard errors are negative codes with a message, never exceptions or crashes: calls out of order,
    null arguments, a model that belongs to another handle, unsupported combinations."""
    lib = _lib.load()
    o = _lib.Options()
    lib.fpsq_default_options(50, 5, C.byref(o))
    h = C.c_void_p()
    assert lib.fpsq_create(C.byref(h), 50, 5, C.byref(o)) == 0
    st = (_lib.Stats * 2)()
    z = np.zeros(50)
    zm = np.zeros(5)
    # solve before the Jacobian structure / values exist
    rc = lib.fpsq_solve_two_mixed(h, z.ctypes.data, zm.ctypes.data, z.ctypes.data, zm.ctypes.data, z.ctypes.data,
                                  zm.ctypes.data, st)
    assert rc == -3 and lib.fpsq_last_error(h)
    A = sp.random(5, 50, density=0.3, random_state=np.random.default_rng(3), format="csr")
    A.sort_indices()
    rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    assert lib.fpsq_set_jacobian_structure_csr(h, rp.ctypes.data, ci.ctypes.data) == 0
    rc = lib.fpsq_solve_two_mixed(h, z.ctypes.data, zm.ctypes.data, z.ctypes.data, zm.ctypes.data, z.ctypes.data,
                                  zm.ctypes.data, st)
    assert rc == -3  # structure but no values yet
    assert lib.fpsq_set_jacobian_values(h, A.data.ctypes.data) == 0
    assert lib.fpsq_set_delta(h, -1.0) < 0  # delta must be >= 0
    assert lib.fpsq_solve_two_mixed(h, None, zm.ctypes.data, z.ctypes.data, zm.ctypes.data, z.ctypes.data,
                                    zm.ctypes.data, st) == -1
    assert lib.fpsq_jac_mul(h, 0, 1.0, None, 0.0, zm.ctypes.data) == -1
    # a QP model created on another handle is rejected
    h2 = C.c_void_p()
    assert lib.fpsq_create(C.byref(h2), 50, 5, C.byref(o)) == 0
    assert lib.fpsq_set_jacobian_structure_csr(h2, rp.ctypes.data, ci.ctypes.data) == 0
    assert lib.fpsq_set_jacobian_values(h2, A.data.ctypes.data) == 0
    q = C.c_void_p()
    ones = np.ones(50)
    assert lib.fpsq_qp_create(h2, ones.ctypes.data, z.ctypes.data, zm.ctypes.data, C.byref(q)) == 0
    fx = C.c_double()
    assert lib.fpsq_qp_objgrad(h, q, z.ctypes.data, 1.0, 1.0, 0.0, None, C.byref(fx), None, None, None, st) == -1
    assert lib.fpsq_qp_hprod(h, q, z.ctypes.data, 1.0, 1.0, 0.0, 2, z.ctypes.data, st) == -1
    assert lib.fpsq_qp_hprod(h2, q, z.ctypes.data, 1.0, 1.0, 0.0, 3, z.ctypes.data, st) == -1   # hessian_approx is 1 or 2
    # and the right pairing works
    assert lib.fpsq_qp_objgrad(h2, q, z.ctypes.data, 1.0, 1.0, 0.0, None, C.byref(fx), None, None, None, st) >= 0
    lib.fpsq_qp_destroy(q)
    lib.fpsq_destroy(h2)
    lib.fpsq_destroy(h)


def test_rank_deficient_jacobian_is_handled_softly(oracle):
    """Two identical constraint rows.  delta > 0: the regularised systems are well posed and must match the exact solve.
    delta = 0: the reference's two back-ends legitimately differ (hard parts); what is required is a
    finite result, matching the C restatement's iteration counts and flags -- never a hang or a hard error."""
    qp = _small_pde(seed=41, n=600, m=40)
    A = qp.scipy_csr().tolil()
    A[7, :] = A[3, :]
    A = sp.csr_matrix(A)
    A.sort_indices()
    rng = np.random.default_rng(8)
    g, c = rng.standard_normal(600), rng.standard_normal(40)
    c[7] = c[3]  # consistent right-hand side
    for delta in (1e-2, 0.0):
        H = _Handle(A, delta=delta)
        p1, q1, p2, q2, rc = H.solve_two_mixed(g, c)
        o = oracle.solve_two_mixed(40, 600, A.indptr, A.indices, A.data, delta, g, c)
        assert rc >= 0 and rc == o[5]
        assert all(np.all(np.isfinite(v)) for v in (p1, q1, p2, q2))
        for k in range(2):
            assert abs(H.st[k].niter - o[4][k].niter) <= 1 and H.st[k].solved == o[4][k].solved
        if delta > 0:
            e = oracle.exact_two_mixed(A, delta, g, c)
            for got, want in zip((p1, q1, p2, q2), e):
                assert _rel(got, want) < 1e-5
        else:  # the minimum-norm property: p1 = P_null(A) g does not depend on the redundant row
            assert np.linalg.norm(A @ p1) <= 1e-6 * np.linalg.norm(g)
            assert np.linalg.norm(A @ p2 - c) <= 1e-5 * np.linalg.norm(c)
        H.close()
