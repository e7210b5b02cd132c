// fpsq_coupled.h -- the coupling terms w x_j x_k of fpsq_band_nlp_create_coupled on the host: the checks, and the index lists the
// k_bcn_* and the CP forms of the k_bn_* kernels (fpsq_band_nlp.hip.h) walk.  A term t = (row, j, k, w) adds w x_j x_k to c_row; j and k are both columns of
// that row of the handle's pattern, so J(x) keeps the pattern.  Host-only: needs neither the device runtime nor a handle
// (tests/coupled_nlp_model.py restates it in numpy).
//   partner lists   per STORED entry e = (p, c): the pairs (column, w) with J(x)_e = a_e + h_e x_c + sum w x_column, in term order;
//                   the same lists per entry of the transposed structure (through t_perm), with the entry's own column.
//   S               the n x n pattern of Wo(y) = sum_t w_t y_row(t) (e_j e_k' + e_k e_j'): symmetric, both triangles, no diagonal,
//                   every row sorted by column.
//   contributors    per entry of S: the pairs (stored row, w), in increasing stored row, with Wo(y)_jk = sum w y_row.
// LONG COLUMNS (fpsq_band_nlp_create_coupled_arrow).  The transposed structure of a handle with long columns has virtual entries
// (t_perm = nnz, the slot behind the stored values): they get an empty partner list and column 0.  A long column coupled to the
// states owns a row of S with up to m entries; given the list of long columns the builder leaves those rows EMPTY in the CSR
// (S_band: what the row kernels walk; a long column stays a column of the other rows) and lists them behind it instead: the
// entries of long row i are [lrp[i], lrp[i + 1]) of the SAME sci / cptr arrays, lrp[0] = srp[n], so an entry's index is its
// value slot whichever part it lies in.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace fpsq {

struct CoupledLists {
  std::vector<int32_t> pptr, pcol;    // nnz + 1, 2 T: partner lists of the stored entries
  std::vector<double> pw;             // 2 T
  std::vector<int32_t> tpptr, tpcol;  // t_nnz + 1, 2 T: of the transposed entries
  std::vector<double> tpw;            // 2 T
  std::vector<int32_t> tcol;          // t_nnz: the column of J a transposed entry lies in
  std::vector<int32_t> srp, sci;      // n + 1, nnz(S)
  std::vector<int32_t> cptr, crow;    // nnz(S) + 1, 2 T: contributor lists
  std::vector<double> cw;             // 2 T
  std::vector<int32_t> lrp;           // long columns + 1: their rows of S behind S_band's entries (lrp[0] = srp[n])
};

// rp / ci: the STORED CSR of the handle (m rows); rinv: the caller's row -> the stored one (null = identity); t_perm: transposed
// entry -> stored entry (t_nnz of them).  The terms are in the caller's row order, 0-based.  Returns "" and fills `out`, or what
// is wrong (without the entry's prefix).  lcols: the nlong long columns whose rows of S are listed apart, strictly ascending.
inline std::string coupled_build(int64_t n, int64_t m, const int32_t* rp, const int32_t* ci, const int32_t* rinv, int64_t t_nnz,
                                 const int32_t* t_perm, int64_t nterms, const int32_t* t_row, const int32_t* t_j,
                                 const int32_t* t_k, const double* t_w, CoupledLists& out, int64_t nlong = 0,
                                 const int32_t* lcols = nullptr) {
  const int64_t nnz = rp[m];
  std::vector<int32_t> lidx;  // column -> its place among the long columns, -1: none (empty without long columns)
  if (nlong > 0) {
    lidx.assign((size_t)n, -1);
    for (int64_t i = 0; i < nlong; ++i) {
      if (lcols[i] < 0 || lcols[i] >= n || (i > 0 && lcols[i] <= lcols[i - 1])) return "the long columns are not ascending columns";
      lidx[lcols[i]] = (int32_t)i;
    }
  }
  auto is_long = [&](int32_t col) { return !lidx.empty() && lidx[col] >= 0; };
  if (nterms < 0 || 2 * nterms > INT32_MAX) return "the number of terms is out of range";
  const size_t T = (size_t)nterms;
  struct Att { int32_t p, ej, ek; };  // the stored row and the two stored entries of a term
  std::vector<Att> att(T);
  auto find = [&](int32_t p, int32_t col) {
    for (int32_t e = rp[p]; e < rp[p + 1]; ++e)
      if (ci[e] == col) return e;
    return (int32_t)-1;
  };
  for (size_t t = 0; t < T; ++t) {
    const std::string who = "term " + std::to_string(t);
    if (t_row[t] < 0 || t_row[t] >= m) return who + ": row " + std::to_string(t_row[t]) + " is out of range";
    for (int32_t col : {t_j[t], t_k[t]})
      if (col < 0 || col >= n) return who + ": column " + std::to_string(col) + " is out of range";
    if (t_j[t] == t_k[t])
      return who + ": j = k = " + std::to_string(t_j[t]) + " (a square x_j^2 belongs to h_vals, not to the coupling terms)";
    const int32_t p = rinv ? rinv[t_row[t]] : t_row[t];
    const int32_t ej = find(p, t_j[t]), ek = find(p, t_k[t]);
    if (ej < 0 || ek < 0)
      return who + ": (" + std::to_string(t_row[t]) + ", " + std::to_string(ej < 0 ? t_j[t] : t_k[t]) +
             ") is not an entry of the handle's pattern";
    att[t] = {p, ej, ek};
  }
  {  // a pair {j, k} twice in a row, in either order
    std::vector<size_t> ord(T);
    for (size_t t = 0; t < T; ++t) ord[t] = t;
    auto key = [&](size_t t, int which) {
      const int32_t lo = std::min(t_j[t], t_k[t]), hi = std::max(t_j[t], t_k[t]);
      return which == 0 ? att[t].p : which == 1 ? lo : hi;
    };
    std::sort(ord.begin(), ord.end(), [&](size_t a, size_t c) {
      for (int w = 0; w < 3; ++w)
        if (key(a, w) != key(c, w)) return key(a, w) < key(c, w);
      return a < c;
    });
    for (size_t i = 1; i < T; ++i) {
      const size_t a = ord[i - 1], c = ord[i];
      if (key(a, 0) == key(c, 0) && key(a, 1) == key(c, 1) && key(a, 2) == key(c, 2))
        return "terms " + std::to_string(a) + " and " + std::to_string(c) + ": the pair {" + std::to_string(key(a, 1)) + ", " +
               std::to_string(key(a, 2)) + "} is listed twice in row " + std::to_string(t_row[a]);
    }
  }
  // partner lists of the stored entries, in term order
  out.pptr.assign((size_t)nnz + 1, 0);
  for (size_t t = 0; t < T; ++t) {
    out.pptr[att[t].ej + 1]++;
    out.pptr[att[t].ek + 1]++;
  }
  for (int64_t e = 0; e < nnz; ++e) out.pptr[e + 1] += out.pptr[e];
  out.pcol.assign(2 * T, 0);
  out.pw.assign(2 * T, 0.0);
  {
    std::vector<int32_t> nxt(out.pptr.begin(), out.pptr.end() - 1);
    for (size_t t = 0; t < T; ++t) {
      int32_t u = nxt[att[t].ej]++;
      out.pcol[u] = t_k[t];
      out.pw[u] = t_w[t];
      u = nxt[att[t].ek]++;
      out.pcol[u] = t_j[t];
      out.pw[u] = t_w[t];
    }
  }
  // the same lists in the transposed order
  out.tpptr.assign((size_t)t_nnz + 1, 0);
  out.tcol.assign((size_t)t_nnz, 0);
  out.tpcol.clear();
  out.tpw.clear();
  out.tpcol.reserve(2 * T);
  out.tpw.reserve(2 * T);
  for (int64_t k = 0; k < t_nnz; ++k) {
    const int32_t e = t_perm[k];
    if (e >= nnz) {  // a virtual entry of a long column: it gathers a = 1, h = 0 and meets no term
      out.tpptr[k + 1] = (int32_t)out.tpcol.size();
      continue;
    }
    out.tcol[k] = ci[e];
    for (int32_t u = out.pptr[e]; u < out.pptr[e + 1]; ++u) {
      out.tpcol.push_back(out.pcol[u]);
      out.tpw.push_back(out.pw[u]);
    }
    out.tpptr[k + 1] = (int32_t)out.tpcol.size();
  }
  // S and its contributor lists: both orientations of every term, sorted by (row of S, column of S, stored row), the rows of
  // the long columns behind all others
  struct Tri { int32_t j, k, p; double w; };
  std::vector<Tri> tri;
  tri.reserve(2 * T);
  for (size_t t = 0; t < T; ++t) {
    tri.push_back({t_j[t], t_k[t], att[t].p, t_w[t]});
    tri.push_back({t_k[t], t_j[t], att[t].p, t_w[t]});
  }
  std::sort(tri.begin(), tri.end(), [&](const Tri& a, const Tri& c) {
    if (is_long(a.j) != is_long(c.j)) return is_long(c.j);
    return a.j != c.j ? a.j < c.j : a.k != c.k ? a.k < c.k : a.p < c.p;
  });
  out.srp.assign((size_t)n + 1, 0);
  out.lrp.assign((size_t)nlong + 1, 0);
  out.sci.clear();
  out.cptr.assign(1, 0);
  out.crow.assign(2 * T, 0);
  out.cw.assign(2 * T, 0.0);
  for (size_t i = 0; i < tri.size(); ++i) {
    if (i == 0 || tri[i].j != tri[i - 1].j || tri[i].k != tri[i - 1].k) {
      if (i) out.cptr.push_back((int32_t)i);
      out.sci.push_back(tri[i].k);
      if (is_long(tri[i].j))
        out.lrp[lidx[tri[i].j] + 1]++;
      else
        out.srp[tri[i].j + 1]++;
    }
    out.crow[i] = tri[i].p;
    out.cw[i] = tri[i].w;
  }
  if (!tri.empty()) out.cptr.push_back((int32_t)tri.size());
  for (int64_t j = 0; j < n; ++j) out.srp[j + 1] += out.srp[j];
  out.lrp[0] = out.srp[n];
  for (int64_t i = 0; i < nlong; ++i) out.lrp[i + 1] += out.lrp[i];
  return "";
}

}  // namespace fpsq
