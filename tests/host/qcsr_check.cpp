// qcsr_check.cpp -- drives csrc/fpsq_qcsr.h, the host-side check and split Q = diag(q) + R of a sparse symmetric objective
// Hessian that fpsq_band_qp_create_csr and fpsq_qp_create_csr share.  Stand-alone (its own main, includes nothing of the
// library but that header and the lane-group rule): symmetric inputs (banded with empty rows, unsorted columns, an absent
// diagonal, n = 1, an empty matrix) must split into a diagonal and an R with sorted rows whose DENSE reconstruction is Q;
// unsymmetric values, an unsymmetric pattern, a duplicate, a column out of range on either side and a bad rowptr must be
// refused with the word the C ABI promises in its message.  tests/test_qp_sparse_hessian_cpu.py compiles and runs it, plain
// and under the address / undefined-behaviour sanitizers.
#include "fpsq_lanegroup.h"
#include "fpsq_qcsr.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

using namespace fpsq;

namespace {

int g_fail = 0;

void fail(const std::string& name, const std::string& what) {
  ++g_fail;
  std::fprintf(stderr, "FAIL [%s] %s\n", name.c_str(), what.c_str());
}

uint64_t g_rng = 0;
uint32_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

struct Csr {
  int64_t n = 0;
  std::vector<int32_t> rp, ci;
  std::vector<double> va;
};

// from (row, column) -> value, rows in ascending column order
Csr from_map(int64_t n, const std::vector<std::map<int32_t, double>>& rows) {
  Csr q;
  q.n = n;
  q.rp.assign((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    for (const auto& e : rows[i]) {
      q.ci.push_back(e.first);
      q.va.push_back(e.second);
    }
    q.rp[i + 1] = (int32_t)q.ci.size();
  }
  return q;
}

// banded symmetric Q of half width hw; rows i with i % 7 == 3 have no off-diagonal entry (their columns neither);
// diag: 0 = absent everywhere, 1 = stored everywhere, 2 = stored on every other row
Csr banded(int64_t n, int hw, int diag, uint64_t seed) {
  g_rng = seed;
  std::vector<std::map<int32_t, double>> rows((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (diag == 1 || (diag == 2 && i % 2 == 0)) rows[i][(int32_t)i] = 1.0 + (rnd() % 1000) / 100.0;
    for (int k = 1; k <= hw; ++k) {
      const int64_t j = i + k;
      if (j >= n || i % 7 == 3 || j % 7 == 3) continue;
      const double v = (rnd() % 2001) / 1000.0 - 1.0;
      rows[i][(int32_t)j] = v;
      rows[j][(int32_t)i] = v;
    }
  }
  return from_map(n, rows);
}

// every row's entries in a random order
void shuffle_rows(Csr& q, uint64_t seed) {
  g_rng = seed;
  for (int64_t i = 0; i < q.n; ++i)
    for (int32_t k = q.rp[i + 1] - 1; k > q.rp[i]; --k) {
      const int32_t j = q.rp[i] + (int32_t)(rnd() % (uint32_t)(k - q.rp[i] + 1));
      std::swap(q.ci[k], q.ci[j]);
      std::swap(q.va[k], q.va[j]);
    }
}

std::string run(const Csr& q, QcsrSplit& sp) {
  const std::string r = qcsr_check_rowptr(q.n, q.rp.data());
  if (!r.empty()) return r;
  return qcsr_check_split(q.n, q.rp.data(), q.ci.data(), q.va.data(), sp);
}

// a symmetric input: accepted, and diag + R reconstructs Q entry for entry (dense, so the cases stay small)
void accept(const std::string& name, const Csr& q) {
  QcsrSplit sp;
  const std::string msg = run(q, sp);
  if (!msg.empty()) return fail(name, "refused: " + msg);
  const size_t n = (size_t)q.n;
  if (sp.qd.size() != n || sp.rrp.size() != n + 1 || sp.rrp[0] != 0 || sp.rci.size() != sp.rv.size() ||
      (size_t)sp.rrp[n] != sp.rci.size())
    return fail(name, "sizes of the split");
  std::vector<double> want(n * n, 0.0), got(n * n, 0.0);
  std::vector<char> stored(n * n, 0), rstored(n * n, 0);
  size_t ndiag = 0;
  for (size_t i = 0; i < n; ++i)
    for (int32_t k = q.rp[i]; k < q.rp[i + 1]; ++k) {
      want[i * n + (size_t)q.ci[k]] = q.va[k];
      stored[i * n + (size_t)q.ci[k]] = 1;
      ndiag += (size_t)q.ci[k] == i;
    }
  for (size_t i = 0; i < n; ++i) {
    got[i * n + i] = sp.qd[i];
    if (sp.rrp[i + 1] < sp.rrp[i]) return fail(name, "row offsets of R decrease");
    for (int32_t k = sp.rrp[i]; k < sp.rrp[i + 1]; ++k) {
      const int32_t j = sp.rci[k];
      if (j < 0 || (size_t)j >= n || (size_t)j == i) return fail(name, "a column of R is out of range or on the diagonal");
      if (k > sp.rrp[i] && sp.rci[k - 1] >= j) return fail(name, "a row of R is not sorted by column");
      got[i * n + (size_t)j] = sp.rv[k];
      rstored[i * n + (size_t)j] = 1;
    }
  }
  if (sp.rci.size() + ndiag != q.ci.size()) return fail(name, "R holds another number of entries than Q off its diagonal");
  for (size_t e = 0; e < n * n; ++e) {
    if (got[e] != want[e]) return fail(name, "diag + R != Q at entry " + std::to_string(e));
    if (e / n != e % n && stored[e] != rstored[e]) return fail(name, "a stored entry (a stored zero?) was dropped from R");
  }
  // the lanes per row the kernels would take: a power of two, 1 .. 64, no more than the mean row length
  const int lg = lane_group((int64_t)sp.rci.size(), q.n);
  if (lg < 1 || lg > 64 || (lg & (lg - 1)) || (lg > 1 && (int64_t)lg * q.n > (int64_t)sp.rci.size())) return fail(name, "lane_group");
  std::printf("  %-28s accepted: n = %lld, nnz(Q) = %zu, nnz(R) = %zu, lanes %d\n", name.c_str(), (long long)q.n, q.ci.size(),
              sp.rci.size(), lg);
}

void refuse(const std::string& name, const Csr& q, const std::string& word) {
  QcsrSplit sp;
  const std::string msg = run(q, sp);
  if (msg.empty()) return fail(name, "accepted");
  if (msg.find(word) == std::string::npos) return fail(name, "'" + msg + "' does not name '" + word + "'");
  std::printf("  %-28s refused:  %s\n", name.c_str(), msg.c_str());
}

}  // namespace

int main() {
  for (int hw : {1, 2, 8}) accept("banded hw=" + std::to_string(hw), banded(61, hw, 1, 11 + hw));
  accept("absent diagonal", banded(45, 2, 0, 3));
  accept("diagonal on every other row", banded(45, 3, 2, 4));
  {
    Csr q = banded(50, 8, 1, 5);
    shuffle_rows(q, 6);
    accept("unsorted columns", q);
  }
  {
    Csr q = banded(40, 2, 1, 7);
    for (auto& v : q.va) v = 0.0;  // stored zeros stay entries of R
    accept("stored zeros", q);
  }
  accept("n = 1", banded(1, 1, 1, 8));
  accept("diagonal only", banded(9, 0, 1, 9));
  {
    Csr q;  // no entry at all: every row of R is empty, the diagonal is zero
    q.n = 5;
    q.rp.assign(6, 0);
    accept("empty matrix", q);
  }
  {
    Csr q;
    q.n = 0;
    q.rp.assign(1, 0);
    accept("n = 0", q);
  }

  const Csr base = banded(30, 2, 1, 21);  // row 7: columns 5 6 7 8 9
  const int32_t k7 = base.rp[7];
  if (base.rp[8] - k7 != 5 || base.ci[k7] != 5) fail("base", "row 7 is not what the cases below assume");
  {
    Csr q = base;
    q.va[k7] += 1e-9;
    refuse("unsymmetric value", q, "values");
  }
  {
    Csr q = base;
    q.ci[k7] = 4;  // (7, 4) has no transpose
    refuse("unsymmetric pattern", q, "pattern");
  }
  {
    Csr q = base;  // an entry in the upper triangle only, in a row that is empty otherwise
    q.ci[base.rp[3]] = 20;
    refuse("unsymmetric pattern (empty row)", q, "pattern");
  }
  {
    Csr q = base;
    q.ci[k7] = q.ci[k7 + 1];
    refuse("duplicate", q, "duplicate");
  }
  {
    Csr q = base;
    shuffle_rows(q, 2);
    q.ci[q.rp[8] - 1] = q.ci[k7];
    refuse("duplicate (unsorted)", q, "duplicate");
  }
  {
    Csr q = base;
    q.ci[k7] = (int32_t)q.n;
    refuse("column n", q, "range");
  }
  {
    Csr q = base;
    q.ci[k7] = -1;
    refuse("column -1", q, "range");
  }
  {
    Csr q = base;
    q.ci[q.ci.size() - 1] = INT32_MAX;
    refuse("column INT32_MAX", q, "range");
  }
  {
    Csr q = base;
    q.rp[0] = 1;
    refuse("rowptr[0] != 0", q, "rowptr");
  }
  {
    Csr q = base;
    q.rp[5] = q.rp[4] - 1;
    refuse("rowptr decreases", q, "rowptr");
  }
  std::printf("%d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}
