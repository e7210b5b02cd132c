"""The coupled quadratic model in numpy, fp64, assembled THE WAY THE DEVICE ASSEMBLES IT (csrc/fpsq_coupled.h: the index lists;
csrc/fpsq_band_nlp.hip.h: the sums of the k_bn_*<LG, true> and k_bcn_* kernels and of the launches they share with the other
models), on a STORED row order of the caller's choice (`rperm`: stored row -> the caller's, what the symbolic phase of a
reordered or two-chain handle does to the rows; columns keep their order):

  * `build_lists` restates coupled_build: every term is attached to its two stored entries through the row permutation, the
    per-entry partner lists (column, w) in term order, the same lists in the transposed order through t_perm, the pattern S of
    Wo (symmetric, full, no diagonal, rows sorted) and per entry of S the contributors (stored row, w) in increasing row;
  * `vals` / `tvals`: J(x) = a + h x_c + sum_partners w x_partner in both orders;
  * the prologue's identity c = sum 1/2 (J + a) x - b (no walk of the term lists), `cons` with the partner lists;
  * the epilogue's six sums, the assembly of -Wo(ys), Wo(q2), Wo(c) on S, the finish sums;
  * Val(2) in bq_launches' sparse form with Q = diag(qe) + R, R = -Wo(ys), then hc .* v + Wo(c) v;
  * Val(1): E in its own epilogue, Wo(q1) from the contributor lists, ghjvprod with the partner lists, the second solve.

The M-solves are exact: one sparse LU of K = [I J'; J -delta I], M^-1 r = the multiplier part of K^-1 (0, -r).  Formulas:
include/fpsq.h fpsq_band_nlp_create_coupled.  Never used by the product; it carries no fitted constant."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def build_lists(n, m, rp, ci, rinv, t_perm, t_row, t_j, t_k, t_w):
    """coupled_build: rp / ci the STORED CSR, rinv the caller's row -> the stored one, t_perm transposed entry -> stored entry.
    Raises ValueError with coupled_build's reason for the terms it refuses."""
    T = len(t_w)
    att = []
    for t in range(T):
        r, j, k = int(t_row[t]), int(t_j[t]), int(t_k[t])
        if not 0 <= r < m:
            raise ValueError(f"term {t}: row {r} is out of range")
        for c in (j, k):
            if not 0 <= c < n:
                raise ValueError(f"term {t}: column {c} is out of range")
        if j == k:
            raise ValueError(f"term {t}: j = k = {j}")
        p = int(rinv[r])
        ent = []
        for c in (j, k):
            hit = [e for e in range(rp[p], rp[p + 1]) if ci[e] == c]
            if not hit:
                raise ValueError(f"term {t}: ({r}, {c}) is not an entry of the handle's pattern")
            ent.append(hit[0])
        att.append((p, ent[0], ent[1]))
    seen = {}
    for t in range(T):
        key = (att[t][0], min(t_j[t], t_k[t]), max(t_j[t], t_k[t]))
        if key in seen:
            raise ValueError(f"terms {seen[key]} and {t}: the pair is listed twice in row {t_row[t]}")
        seen[key] = t
    nnz = int(rp[m])
    partners = [[] for _ in range(nnz)]                       # per stored entry: (column, w), in term order
    for t in range(T):
        p, ej, ek = att[t]
        partners[ej].append((int(t_k[t]), float(t_w[t])))
        partners[ek].append((int(t_j[t]), float(t_w[t])))
    t_partners = [partners[e] for e in t_perm]                # per transposed entry, through t_perm
    tcol = np.asarray(ci)[t_perm]
    tri = sorted([(int(t_j[t]), int(t_k[t]), att[t][0], float(t_w[t])) for t in range(T)] +
                 [(int(t_k[t]), int(t_j[t]), att[t][0], float(t_w[t])) for t in range(T)], key=lambda u: u[:3])
    srp, sci, contrib = np.zeros(n + 1, dtype=np.int64), [], []
    for i, (j, k, p, w) in enumerate(tri):
        if i == 0 or tri[i - 1][:2] != (j, k):
            sci.append(k)
            contrib.append([])
            srp[j + 1] += 1
        contrib[-1].append((p, w))
    return dict(partners=partners, t_partners=t_partners, tcol=tcol, srp=np.cumsum(srp), sci=np.asarray(sci, dtype=np.int64),
                contrib=contrib)


class CoupledNLPModel:
    def __init__(self, data, rperm=None):
        qp = data.qp
        self.data, self.qp = data, qp
        n, m = qp.n, qp.m
        self.rperm = np.arange(m) if rperm is None else np.asarray(rperm, dtype=np.int64)
        rinv = np.empty(m, dtype=np.int64)
        rinv[self.rperm] = np.arange(m)
        # the stored CSR: rows in the stored order, entries of a row in the caller's order (vperm: stored entry -> the caller's)
        lens = np.diff(qp.rowptr)[self.rperm]
        self.rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.vperm = np.concatenate([np.arange(qp.rowptr[r], qp.rowptr[r + 1]) for r in self.rperm]).astype(np.int64)
        self.ci = qp.colind[self.vperm].astype(np.int64)
        self.rows = np.repeat(np.arange(m), lens)
        self.a, self.h = qp.vals[self.vperm], data.hvals[self.vperm]
        self.bp = data.b[self.rperm]
        # the transposed structure: entries by column, then by stored row
        self.t_perm = np.lexsort((self.rows, self.ci))
        self.t_rp = np.concatenate([[0], np.cumsum(np.bincount(self.ci, minlength=n))])
        self.t_ci = self.rows[self.t_perm]
        self.ta, self.th = self.a[self.t_perm], self.h[self.t_perm]
        self.L = build_lists(n, m, self.rp, self.ci, rinv, self.t_perm, data.t_row, data.t_j, data.t_k, data.t_w)
        self.srow = np.repeat(np.arange(n), np.diff(self.L["srp"]))

    # ---- J(x) in both orders (k_bcn_vals, twice)
    @staticmethod
    def _vals(a, h, col, partners, x):
        out = a + h * x[col]
        for k, lst in enumerate(partners):
            for c, w in lst:
                out[k] += w * x[c]
        return out

    def vals(self, x):
        return self._vals(self.a, self.h, self.ci, self.L["partners"], x)

    def tvals(self, x):
        return self._vals(self.ta, self.th, self.L["tcol"], self.L["t_partners"], x)

    def _J(self, vals):
        return sp.csr_matrix((vals, self.ci, self.rp), shape=(self.qp.m, self.qp.n))

    def _Jt(self, tvals):
        return sp.csr_matrix((tvals, self.t_ci, self.t_rp), shape=(self.qp.n, self.qp.m))

    def cons(self, x):
        """k_bn_cons<LG, true>: from the model's own arrays, every term met at both of its entries, half each; the caller's rows"""
        ps = np.array([sum(w * x[c] for c, w in lst) for lst in self.L["partners"]])
        xv = x[self.ci]
        s = np.bincount(self.rows, (self.a + 0.5 * self.h * xv + 0.5 * ps) * xv, self.qp.m) - self.bp
        out = np.empty(self.qp.m)
        out[self.rperm] = s
        return out

    def _on_s(self, y):
        """Wo(y) on S from the contributor lists (y in the stored row order)"""
        return np.array([sum(w * y[p] for p, w in lst) for lst in self.L["contrib"]])

    def _s_mul(self, svals, v):
        return np.bincount(self.srow, svals * v[self.L["sci"]], self.qp.n)

    def _msolve(self, R):
        n, m = self.qp.n, self.qp.m
        return np.column_stack([self.lu.solve(np.concatenate([np.zeros(n), -R[:, k]]))[n:] for k in range(R.shape[1])])

    def objgrad(self, x, sigma, rho, delta, eta=0.0, xk=None):
        """dict(fx, gx, ys, gs, c); leaves what an hprod runs on"""
        qp = self.qp
        n, m = qp.n, qp.m
        x = np.asarray(x, float)
        jv, jt = self.vals(x), self.tvals(x)
        assert np.array_equal(jt, jv[self.t_perm])              # the two value arrays hold the same bits
        J, Jt = self._J(jv), self._Jt(jt)
        self.J, self.Jt = J, Jt
        self.lu = spla.splu(sp.bmat([[sp.identity(n), J.T], [J, -float(delta) * sp.identity(m)]], format="csc"))
        g = qp.qdiag * x + qp.d
        c = self._J(0.5 * (jv + self.a)) @ x - self.bp          # the prologue's identity
        Y = self._msolve(np.column_stack([J @ g, -c]))
        q1, q2 = Y[:, 0], Y[:, 1]
        Ht = self._Jt(self.th)
        s1, s2, s3 = Jt @ q1, Jt @ q2, Jt @ c
        h1, h2, h3 = Ht @ q1, Ht @ q2, Ht @ c
        gs, p2 = g - s1 - sigma * s2, -s2
        qe = qp.qdiag - (h1 + sigma * h2)
        dx = (x - (np.zeros(n) if xk is None else xk)) if eta > 0.0 else np.zeros(n)
        ys = q1 + sigma * q2
        gx = gs + (sigma - qe) * p2 + h2 * gs + rho * s3 + eta * dx
        rv, wq2, wc = -self._on_s(ys), self._on_s(q2), self._on_s(c)       # the assembly launch
        gx = gx + self._s_mul(wq2, gs) - self._s_mul(rv, p2)                # the finish launch
        fx = x @ (0.5 * qp.qdiag * x + qp.d) - c @ ys + 0.5 * rho * (c @ c) + 0.5 * eta * (dx @ dx)
        self.qe, self.hc, self.gs, self.rv, self.wc = qe, h3, gs, rv, wc
        out_ys, out_c = np.empty(m), np.empty(m)
        out_ys[self.rperm], out_c[self.rperm] = ys, c
        return {"fx": fx, "gx": gx, "ys": out_ys, "gs": gs, "c": out_c}

    def hprod(self, v, sigma, rho, eta, hessian_approx):
        """at the point of the last objgrad"""
        qe, hc, gs, rv, wc = self.qe, self.hc, self.gs, self.rv, self.wc
        J, Jt = self.J, self.Jt
        v = np.asarray(v, float)
        Ev = qe * v + self._s_mul(rv, v)                        # k_bq_pack_sq<HP>: {v, (diag(qe) + R) v}
        Jv = J @ v
        Y = self._msolve(np.column_stack([Jv, J @ Ev]))
        q1 = Y[:, 0]
        s1, s2, s3 = Jt @ q1, Jt @ Y[:, 1], Jt @ Jv
        if hessian_approx == 2:
            Hv = (Ev - s2) - qe * s1 + 2.0 * sigma * s1 + rho * s3 + eta * v    # k_bq_epilogue_sq<HP>, tv = s1
            Hv = Hv - self._s_mul(rv, s1)                                       # k_bq_jacmul on R, alpha = -1
            if rho > 0.0:
                Hv = Hv + (hc * v + self._s_mul(wc, v))                         # k_bcn_hcv
            return Hv
        h1 = self._Jt(self.th) @ q1
        Hv = (Ev - s2) - qe * s1 + 2.0 * sigma * s1 + rho * (s3 + hc * v) + eta * v - h1 * gs   # k_bn_epilogue_h1<LG, true>
        wq1 = self._on_s(q1)
        Hv = Hv + (rho * self._s_mul(wc, v) - self._s_mul(rv, s1) - self._s_mul(wq1, gs))      # k_bcn_finish_h1
        t = self.h * v[self.ci] + np.array([sum(w * v[c] for c, w in lst) for lst in self.L["partners"]])
        ssv = np.bincount(self.rows, gs[self.ci] * t, self.qp.m)                                # k_bn_hgv<LG, true>
        z = self._msolve(ssv[:, None])[:, 0]
        return Hv - Jt @ z                                                                       # k_bn_jtz
