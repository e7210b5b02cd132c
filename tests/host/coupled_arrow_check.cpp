// coupled_arrow_check.cpp -- drives the builder of csrc/fpsq_coupled.h WITH the list of long columns, as
// fpsq_band_nlp_create_coupled_arrow calls it on a handle with long columns: t_perm may hold virtual entries (= nnz, the slot
// behind the stored values; ci and pptr are allocated at their exact sizes, so a sanitized build sees an index past them) and the
// long columns' rows of S are listed apart.  No GPU, no library.  tests/test_band_coupled_arrow_nlp_cpu.py builds it plain and
// under the address / undefined-behaviour sanitizers and compares what it prints with tests/coupled_arrow_nlp_model.py.
//
//   coupled_arrow_check FILE      FILE holds whitespace-separated integers and doubles:
//       n m t_nnz T nlong   rp[m + 1]   ci[nnz]   rinv[m]   t_perm[t_nnz]   lcols[nlong]   then T times: row j k w
//   stdout: "error <message>", or one line per list: the name, its length, its items (%d resp. %.17g)
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "fpsq_coupled.h"

template <class T>
static void put(const char* name, const std::vector<T>& v) {
  std::cout << name << " " << v.size();
  for (const T& a : v) {
    if constexpr (std::is_same<T, double>::value) {
      char buf[40];
      std::snprintf(buf, sizeof buf, " %.17g", a);
      std::cout << buf;
    } else {
      std::cout << " " << a;
    }
  }
  std::cout << "\n";
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  long long n, m, tnz, T, nlong;
  if (!(in >> n >> m >> tnz >> T >> nlong)) return 2;
  std::vector<int32_t> rp(m + 1);
  for (auto& a : rp) in >> a;
  std::vector<int32_t> ci(rp[m]), rinv(m), tperm(tnz), lcols(nlong), row(T), cj(T), ck(T);
  std::vector<double> w(T);
  for (auto& a : ci) in >> a;
  for (auto& a : rinv) in >> a;
  for (auto& a : tperm) in >> a;
  for (auto& a : lcols) in >> a;
  for (long long t = 0; t < T; ++t) in >> row[t] >> cj[t] >> ck[t] >> w[t];
  if (!in) return 2;
  fpsq::CoupledLists L;
  const std::string what = fpsq::coupled_build(n, m, rp.data(), ci.data(), rinv.data(), tnz, tperm.data(), T, row.data(), cj.data(),
                                               ck.data(), w.data(), L, nlong, lcols.data());
  if (!what.empty()) {
    std::cout << "error " << what << "\n";
    return 0;
  }
  put("pptr", L.pptr);
  put("pcol", L.pcol);
  put("pw", L.pw);
  put("tpptr", L.tpptr);
  put("tpcol", L.tpcol);
  put("tpw", L.tpw);
  put("tcol", L.tcol);
  put("srp", L.srp);
  put("sci", L.sci);
  put("cptr", L.cptr);
  put("crow", L.crow);
  put("cw", L.cw);
  put("lrp", L.lrp);
  return 0;
}
