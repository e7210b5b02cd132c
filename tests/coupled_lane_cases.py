"""Shapes built to run the row kernels of the coupled quadratic model (fpsq_band_nlp_create_coupled, DeviceBandCoupledQuadNLP:
k_bn_cons / k_bn_prologue / k_bn_epilogue / k_bn_epilogue_h1 / k_bn_hgv as <LG, true>, k_bcn_finish, k_bcn_hcv,
k_bcn_finish_h1 and k_bq_pack_sq<LG, true>) at EVERY lane-group width on each of their three sides, and k_bcn_assemble through
the second trip of its grid-stride loop; shared by tests/test_coupled_lane_groups_cpu.py (no GPU) and
tests/test_gpu_coupled_lane_groups.py.  Test infrastructure, in the manner of tests/coupled_cases.py, whose cases reach
lgA 2, 4, 16, 32, lgT 1, 2, 32 and lgR 1, 8 only.

THE TERM RULE (with_reach).  problems.with_coupled_constraints couples neighbouring entries and never gets past lgR = 16 on the
shapes of tests/lane_group_cases.py; lgR = lane_group(nnz(S), n) needs rows of S as long as the rows of A'.  Here every row
with entries e_0 < ... < e_{L-1} gets every pair (e_u, e_{u+s}), 1 <= s <= reach, the terms sorted by (row, first entry, second
entry); hvals are those of with_quadratic_constraints(qp, curv, seed); weights curv / sqrt(reach) sqrt|a_j a_k| U(0.5, 1.5) (+-1)
from default_rng(seed + 1) (every U, then every sign); b through problems._coupled, so xhat stays feasible.  An entry has up to
2 reach partners, each of weight ~ curv / sqrt(reach) |a|: the 1 / sqrt(reach) keeps the partner sums, and with them J(x), of
the size the separable curvature gives them (sigma_min(J(x)) is printed and bounded by the CPU test).

CASES: a shape of tests/lane_group_cases.py (its lgA / lgT) and a reach; CURV = 0.3, seed 7
  case                  lgA lgT  reach  lgR  nnz(S)    terms     there for
  thin-r2               1   1    2      1    798       400       one lane on all three sides; rows of one entry: no term
  lg2-r4                2   1    4      1    1594      800       A at 2
  lg4-2-r1              4   2    1      2    4092      2100      4 / 2 / 2
  lg4-2-r2              4   2    2      4    6958      3600      S at 4
  lg8-4-r3              8   4    3      16   82626     45000     8 / 4
  lg16-2-r8             16  2    8      16   54034     31000     A at 16
  lgT-8-r2              32  8    2      16   27284     26070     A' at 8
  lgT-16-r4             32  16   4      32   34370     75000     A' at 16, S at 32
  m-near-n-r1           32  32   1      8    12074     39000     S at 8
  both-64-r16           64  64   16     64   38432     572000    64 lanes on all three sides
  wide-rows-r1          64  8    1      4    9210      15264     A at 64 with A' at 8
  ragged-r2             32  32   2      16   41028     117125    rows of one entry without a term next to rows of 200 with 397
  both-64-shuffled-r16  64  64   16     64   38432     572000    a reordered handle: the terms' rows go through the permutation
  ragged-shuffled-r2    32  32   2      16   41028     117125    the same at 32 lanes
  assemble-stride       64  8    159    64   1664120   2035200   k_bcn_assemble's second trip (below)
Together: lgA, lgT and lgR each take every width 1, 2, 4, 8, 16, 32, 64 (the CPU test recomputes the three sets).

ASSEMBLE-STRIDE.  lane_group_cases.ragged_band(2048, 160, (160,), 640, 31) with reach = 159: every pair of every row, so the
pattern of S does not depend on the draws.  nnz(S) = 1664120 > 4096 x 256: k_bcn_assemble, a thread per entry of S under the
flat-grid cap of 4096 workgroups, would take 6501 workgroups and walks a second trip -- the only case of any suite that does
(tests/coupled_cases.py's STRIDE has one term per row: that rule would need N > 524288).  The longest row of S has 1186 entries
(18 trips of a 64-lane group).  It runs at one delta and one (rho, eta), rho > 0: Wo(c), the third array the kernel writes, is
read by hprod under rho > 0 only.

YARDSTICK.  expected(name, delta): tests/coupled_quad_ref.py with kept factors (exact sparse KKT solves at J(x), fp64, no
device code), at x = qp.x, xk = qp.xhat, once per case and delta, read-only."""
import dataclasses
import functools

import numpy as np

from fps_amd import problems
import coupled_cases as cc
import lane_group_cases as L

SE, SIGMA, CURV, SEED = L.SE, L.SIGMA, L.CURV, 7
WIDTHS = L.WIDTHS
RHO_ETA = ((0.0, 0.0), (1.0, 0.5))
STRIDE = "assemble-stride"


def with_reach(qp, curv, reach, seed):
    """the term rule of the module docstring on `qp`"""
    sep = problems.with_quadratic_constraints(qp, curv, seed)
    rowptr = qp.rowptr.astype(np.int64)
    lens = np.diff(rowptr)
    rows = np.repeat(np.arange(qp.m, dtype=np.int64), lens)
    eid = np.arange(qp.nnz, dtype=np.int64)
    after = rowptr[rows + 1] - 1 - eid                       # entries of the row behind this one
    cnt = np.minimum(after, int(reach))
    e_j = np.repeat(eid, cnt)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    e_k = e_j + 1 + (np.arange(e_j.size, dtype=np.int64) - np.repeat(first, cnt))
    rng = np.random.default_rng(seed + 1)
    t_w = (curv / np.sqrt(reach) * np.sqrt(np.abs(qp.vals[e_j] * qp.vals[e_k])) * rng.uniform(0.5, 1.5, e_j.size)
           * rng.choice([-1.0, 1.0], e_j.size))
    return problems._coupled(qp, sep.hvals, rows[e_j], qp.colind[e_j], qp.colind[e_k], t_w)


@dataclasses.dataclass(frozen=True)
class Case:
    """A shape, a reach and the literals tests/test_coupled_lane_groups_cpu.py pins on them."""
    base: str             # a case of tests/lane_group_cases.py; None: the shape of assemble-stride
    reach: int
    lgA: int
    lgT: int
    lgR: int
    snz: int              # nnz(S)
    nterms: int
    longest: int          # the longest row of S
    band: dict            # what the handle's info() must say: chains, nblocks, bandwidth_blocks, reordered


def _case(base, reach, lgR, snz, nterms, longest):
    c = L.CASES[base]
    return Case(base, reach, c.lgA, c.lgT, lgR, snz, nterms, longest, c.band)


CASES = {
    "thin-r2": _case("thin", 2, 1, 798, 400, 8),
    "lg2-r4": _case("lg2", 4, 1, 1594, 800, 13),
    "lg4-2-r1": _case("lg4-2", 1, 2, 4092, 2100, 11),
    "lg4-2-r2": _case("lg4-2", 2, 4, 6958, 3600, 18),
    "lg8-4-r3": _case("lg8-4", 3, 16, 82626, 45000, 64),
    "lg16-2-r8": _case("lg16-2", 8, 16, 54034, 31000, 70),
    "lgT-8-r2": _case("lgT-8", 2, 16, 27284, 26070, 29),
    "lgT-16-r4": _case("lgT-16", 4, 32, 34370, 75000, 36),
    "m-near-n-r1": _case("m-near-n", 1, 8, 12074, 39000, 12),
    "both-64-r16": _case("both-64", 16, 64, 38432, 572000, 66),
    "wide-rows-r1": _case("wide-rows", 1, 4, 9210, 15264, 7),
    "ragged-r2": _case("ragged", 2, 16, 41028, 117125, 57),
    "both-64-shuffled-r16": _case("both-64-shuffled", 16, 64, 38432, 572000, 66),
    "ragged-shuffled-r2": _case("ragged-shuffled", 2, 16, 41028, 117125, 57),
    STRIDE: Case(None, 159, 64, 8, 64, 1664120, 2035200, 1186, dict(chains=1, nblocks=2, bandwidth_blocks=1, reordered=0)),
}
NAMES = list(CASES)
STRIDE_SHAPE = (2048, 160, (160,), 640, 31)      # ragged_band's arguments
DELTA0 = ("thin-r2", "lg2-r4", "lg4-2-r2")       # the cases that run at delta = 0 too


def deltas(name):
    return (0.0, SE) if name in DELTA0 else (SE,)


def pairs(name):
    """the (rho, eta) a case runs at"""
    return RHO_ETA[1:] if name == STRIDE else RHO_ETA


@functools.lru_cache(maxsize=None)
def data(name):
    """the CoupledQuadNLP of a case (shared, read-only)"""
    c = CASES[name]
    qp = L.ragged_band(*STRIDE_SHAPE) if c.base is None else L.qp(c.base)
    out = with_reach(qp, CURV, c.reach, SEED)
    for a in (out.hvals, out.b, out.t_row, out.t_j, out.t_k, out.t_w, out.qp.vals, out.qp.x, out.qp.xhat):
        a.setflags(write=False)
    return out


def lanes(d):
    """(lgA, lgT, lgR, nnz(S), the longest row of S) recomputed from the model"""
    _, snz, longest = cc.s_pattern(d)
    qp = d.qp
    return L.lane_group(qp.nnz, qp.m), L.lane_group(qp.nnz, qp.n), L.lane_group(snz, qp.n), snz, longest


def v_of(qp):
    return np.random.default_rng(0).standard_normal(qp.n)


@functools.lru_cache(maxsize=None)
def expected(name, delta):
    """what the yardstick says at x = qp.x, xk = qp.xhat: {(rho, eta): dict(fx, gx, ys, gs, c, Hv2, Hv1)} over pairs(name),
    computed once and left unchanged"""
    from coupled_quad_ref import CoupledQuadRef

    d = data(name)
    qp = d.qp
    ref = CoupledQuadRef(d, SIGMA, 0.0, delta, 0.0, qp.xhat, keep_factors=True)
    out = {}
    for rho, eta in pairs(name):
        ref.pen.rho, ref.pen.eta = rho, eta
        e = dict(ref.objgrad(qp.x))
        e["Hv2"], e["Hv1"] = ref.hprod(qp.x, v_of(qp), 2), ref.hprod(qp.x, v_of(qp), 1)
        for a in e.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[(rho, eta)] = e
    return out
