"""The coupled quadratic model on a handle with LONG COLUMNS in numpy, fp64: tests/coupled_nlp_model.py with what
fpsq_band_nlp_create_coupled_arrow adds to it, assembled the way the device assembles it (csrc/fpsq_coupled.h: the lists;
csrc/fpsq_band.hip.h k_bq_long_rows: the sums):

  * `build_lists_arrow` restates the extended coupled_build: the transposed structure of such a handle holds, in the row of a long
    column, `vgrid` VIRTUAL entries (t_perm = nnz) in the place of the column's own; they get an empty partner list and column 0
    and gather a = 1, h = 0, so they evaluate to 1 at every x (`dev_tvals`).  The rows of S that long columns own are EMPTY in
    the CSR (`srp`) and listed behind its entries in the same `sci` / `contrib` arrays, long row i at [lrp[i], lrp[i + 1]): an
    entry's index is its value slot in either part;
  * `_s_mul`, through which every product with Wo(ys), Wo(q2), Wo(c), Wo(q1) of CoupledNLPModel goes -- the finish sums of an
    objgrad, (R v) of the pack, R Ptv and Wo(c) v of Val(2), the three of Val(1) --, forms the rows of the CSR and then EACH LONG
    ROW on its own, entry by entry, and adds it at the long column (k_bq_long_rows' four modes); `long_rows=False` leaves those
    sums out, which is what the CSR alone gives.

Everything else is CoupledNLPModel's: exact M-solves on K = [I J'; J -delta I] (the arrow scheme of the handle's own solves is
tests/arrow_nlp_model.py's subject) and its J' / H' sums over the real transposed structure.  Never used by the product; it
carries no fitted constant."""
import numpy as np

from coupled_nlp_model import CoupledNLPModel, build_lists


def device_t_perm(n, ci, rows, nnz, lcols, vgrid):
    """t_perm of a handle with long columns: by column, then stored row; a long column's row holds vgrid virtual entries"""
    real = np.lexsort((rows, ci))
    lc = set(int(c) for c in lcols)
    out, at = [], 0
    counts = np.bincount(ci, minlength=n)
    for j in range(n):
        if j in lc:
            out.extend([nnz] * vgrid)
        else:
            out.extend(real[at:at + counts[j]].tolist())
        at += counts[j]
    return np.asarray(out, dtype=np.int64)


def build_lists_arrow(n, m, rp, ci, rinv, t_perm, t_row, t_j, t_k, t_w, lcols):
    """the extended coupled_build: t_perm may hold virtual entries (= nnz); lcols: the long columns whose rows of S are listed
    apart, ascending"""
    nnz = int(rp[m])
    t_perm = np.asarray(t_perm, dtype=np.int64)
    base = build_lists(n, m, rp, ci, rinv, t_perm[t_perm < nnz], t_row, t_j, t_k, t_w)
    t_partners, tcol = [], []
    for e in t_perm:
        virtual = e >= nnz
        t_partners.append([] if virtual else base["partners"][e])
        tcol.append(0 if virtual else int(ci[e]))
    lcols = [int(c) for c in lcols]
    assert all(a < b for a, b in zip(lcols, lcols[1:]))
    srp, sci, contrib = base["srp"], base["sci"], base["contrib"]
    band_rp, order, lrp = np.zeros(n + 1, dtype=np.int64), [], []
    for j in range(n):
        if j not in lcols:
            order.extend(range(srp[j], srp[j + 1]))
        band_rp[j + 1] = len(order)
    for j in lcols:
        lrp.append(len(order))
        order.extend(range(srp[j], srp[j + 1]))
    lrp.append(len(order))
    return dict(partners=base["partners"], t_partners=t_partners, tcol=np.asarray(tcol, dtype=np.int64), srp=band_rp,
                sci=sci[order] if len(order) else sci, contrib=[contrib[k] for k in order], lrp=np.asarray(lrp, dtype=np.int64),
                lcols=np.asarray(lcols, dtype=np.int64))


class CoupledArrowNLPModel(CoupledNLPModel):
    def __init__(self, data, lcols, rperm=None, vgrid=3, long_rows=True):
        super().__init__(data, rperm)
        qp = data.qp
        rinv = np.empty(qp.m, dtype=np.int64)
        rinv[self.rperm] = np.arange(qp.m)
        self.dev_t_perm = device_t_perm(qp.n, self.ci, self.rows, self.ci.size, lcols, vgrid)
        A = build_lists_arrow(qp.n, qp.m, self.rp, self.ci, rinv, self.dev_t_perm, data.t_row, data.t_j, data.t_k, data.t_w,
                              sorted(int(c) for c in lcols))
        self.A = A
        # the algebra of the parent runs on the REAL transposed structure (L["t_partners"], L["tcol"] stay); S is the split one
        self.L.update(srp=A["srp"], sci=A["sci"], contrib=A["contrib"])
        self.srow = np.repeat(np.arange(qp.n), np.diff(A["srp"]))     # the entries of the CSR alone
        self.long_rows = long_rows

    def dev_tvals(self, x):
        """k_bcn_vals on the handle's transposed structure: the virtual entries gather the slot behind the stored values"""
        a, h = np.append(self.a, 1.0), np.append(self.h, 0.0)
        return self._vals(a[self.dev_t_perm], h[self.dev_t_perm], self.A["tcol"], self.A["t_partners"], x)

    def _s_mul(self, svals, v):
        sci, lrp = self.L["sci"], self.A["lrp"]
        nb = int(self.L["srp"][-1])
        out = np.bincount(self.srow, svals[:nb] * v[sci[:nb]], self.qp.n)
        if self.long_rows:
            for i, T in enumerate(self.A["lcols"]):               # one workgroup per long column
                s = 0.0
                for k in range(lrp[i], lrp[i + 1]):
                    s += svals[k] * v[sci[k]]
                out[T] += s
        return out
