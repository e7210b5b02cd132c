// fpsq_qcsr.h -- a sparse symmetric objective Hessian Q as the *_qp_create_csr entries receive it (n x n CSR, 0-based, both
// triangles, columns in any order, an absent diagonal = 0): the checks and the split Q = diag(q) + R, R in full symmetric row
// storage with every row sorted by column.  Host-only: needs neither the device runtime nor a handle (tests/host/qcsr_check.cpp
// drives it under the sanitizers); fpsq_band_qp_create_csr and fpsq_qp_create_csr both call it on host copies of the arrays.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace fpsq {

struct QcsrSplit {
  std::vector<double> qd;     // n: the diagonal (0 where Q stores none)
  std::vector<int32_t> rrp;   // n + 1: row offsets of R
  std::vector<int32_t> rci;   // columns of R, ascending in every row
  std::vector<double> rv;     // values of R
};

// rowptr alone (before the caller knows how many entries to fetch): "" or what is wrong with it
inline std::string qcsr_check_rowptr(int64_t n, const int32_t* rp) {
  if (rp[0] != 0) return "rowptr[0] must be 0";
  for (int64_t i = 0; i < n; ++i)
    if (rp[i + 1] < rp[i]) return "rowptr decreases at row " + std::to_string(i);
  return "";
}

// The kernels read rows only, so an unsymmetric Q would give a wrong Hessian silently: an index out of range, a duplicate entry,
// a pattern or values that are not symmetric are refused.  Returns "" and fills `out`, or the message (without the entry's
// prefix).  rp has passed qcsr_check_rowptr; ci / va hold rp[n] entries (may be null when that is 0).
inline std::string qcsr_check_split(int64_t n, const int32_t* rp, const int32_t* ci, const double* va, QcsrSplit& out) {
  const size_t nnz = (size_t)rp[n];
  std::vector<std::pair<int32_t, double>> ent(nnz);  // every row sorted by column
  for (int64_t i = 0; i < n; ++i) {
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
      if (ci[k] < 0 || ci[k] >= n)
        return "column " + std::to_string(ci[k]) + " of row " + std::to_string(i) + " is out of range";
      ent[k] = {ci[k], va[k]};
    }
    std::sort(ent.begin() + rp[i], ent.begin() + rp[i + 1],
              [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& c) { return a.first < c.first; });
    for (int32_t k = rp[i] + 1; k < rp[i + 1]; ++k)
      if (ent[k].first == ent[k - 1].first)
        return "duplicate entry (" + std::to_string(i) + ", " + std::to_string(ent[k].first) + ")";
  }
  out.qd.assign((size_t)n, 0.0);
  out.rrp.assign((size_t)n + 1, 0);
  out.rci.clear();
  out.rv.clear();
  out.rci.reserve(nnz);
  out.rv.reserve(nnz);
  for (int64_t i = 0; i < n; ++i) {
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
      const int32_t j = ent[k].first;
      if (j == i) {
        out.qd[i] = ent[k].second;
        continue;
      }
      const auto lo = ent.begin() + rp[j], hi = ent.begin() + rp[j + 1];
      const auto it = std::lower_bound(lo, hi, (int32_t)i,
                                       [](const std::pair<int32_t, double>& a, int32_t col) { return a.first < col; });
      if (it == hi || it->first != i)
        return "the pattern is not symmetric: (" + std::to_string(i) + ", " + std::to_string(j) + ") has no transpose";
      if (!(it->second == ent[k].second))
        return "the values are not symmetric: Q(" + std::to_string(i) + ", " + std::to_string(j) + ") != Q(" +
               std::to_string(j) + ", " + std::to_string(i) + ")";
      out.rci.push_back(j);
      out.rv.push_back(ent[k].second);
    }
    out.rrp[i + 1] = (int32_t)out.rci.size();
  }
  return "";
}

}  // namespace fpsq
