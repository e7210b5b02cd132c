// fpsq_band.hip -- host side of the banded direct back-end (C ABI: include/fpsq.h, "band" section): the symbolic phase
// (ordering, two elimination chains), the block-banded factorisation and the solves, the device-resident eq-QP model
// (fpsq_band_qp_*), the model with nonlinear constraints, separable or with coupling terms (fpsq_band_nlp_*:
// fpsq_band_nlp.hip.h) and the block entries.
#include "fpsq_band.hip.h"
#include "fpsq_qcsr.h"

using namespace fpsq;
using namespace fpsq_direct;

struct fpsq_band_s : DirectCore {
  int64_t nnz = 0;
  int band_w = 1;  // blocks per block row of the band storage = half bandwidth (in blocks) + 1
  int span = 0;    // widest column span of a row (LDS window of k_band_form)
  // row reordering chosen by the symbolic phase (reverse Cuthill-McKee on the rows of A, adjacent = sharing a column):
  // row p of the stored structure is row rperm[p] of the caller's; vperm maps stored entries to the caller's
  bool reordered = false;
  std::vector<int32_t> rperm_host;
  // two elimination chains (see fpsq_band_create): blocks 2 c / 2 c + 1, c < chain_safe, are eliminated side by side on
  // two streams; their couplings reach chain_bw blocks of the same chain (stride 2 in the stored order)
  int chain_safe = 0, chain_bw = 0;
  int32_t *rperm = nullptr, *vperm = nullptr;
  const int32_t* row_perm() const { return reordered ? rperm : nullptr; }  // what the kernels take: null = identity
  double *vals_in = nullptr, *in_bp = nullptr;
  int form_gen = 2, form_R = 1;  // 2: k_band_form_t (by columns of A, form_R rows per pass); 1: k_band_form (row pairs)
  int32_t *rowptr = nullptr, *colind = nullptr, *t_rowptr = nullptr, *t_colind = nullptr, *t_perm = nullptr;
  int2* rowspan = nullptr;
  double *vals = nullptr, *t_vals = nullptr;
  double* Mb = nullptr;    // nb x band_w blocks of 128 x 128
  double *xn = nullptr, *ym = nullptr, *atq = nullptr;  // [n][2], [mpad][2], [n][2]
  hipStream_t stream2 = nullptr;  // the second elimination chain
  hipEvent_t evA = nullptr, evB = nullptr;
  double* csr_in = nullptr;  // fpsq_band_create_coo: the CSR slots the sorted COO entries are summed into
  // block entries (fpsq_band_*_block), allocated when first needed: the interleaved tile A multiplies [n][16], A v [mpad][8],
  // Ptv [n][8] (sparse Q only), and the staging of host-resident blocks (rhs1 / V / X, rhs2 / D, p1 / HV / GX, p2 / GS: 8 n;
  // q1 / YS, q2 / Bv: 8 m; XK: 8 n)
  double *blk_xg = nullptr, *blk_keep = nullptr, *blk_tv = nullptr;
  double* blk_stage[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // fpsq_band_qp_objgrad_block, allocated by its first call: the per-column partial sums of the three product kernels
  // ([kBqMaxGrid][8], [kBqMaxGrid][8][2] twice), the scalars of a tile ([8][5]) and their pinned host side, one slot per tile
  double *og_partF = nullptr, *og_partP = nullptr, *og_partE = nullptr, *og_scal = nullptr, *og_scal_host = nullptr;
  int og_tiles = 0;  // slots of og_scal_host
  bool have_vals = false;    // a factorisation has put the Jacobian's values into vals / t_vals (fpsq_band_jac_mul, fpsq_band_qp_*)
  // bordered band (fpsq_band_create_bordered; kernels and algebra: fpsq_band.hip.h "bordered band"): the last `border` stored
  // rows are eliminated after the band of the first mb = m - border rows; nb, band_w, Mb and the sweeps describe that band
  // alone, mpad pads m.  bd_c / bd_z: C and Z = B^-1 C, [mpad][16]; bd_l: the factor of S, [16][16]; bd_part: the partial
  // sums of a correction, [bd_grid][256]; bd_t: the border's right-hand side while its slots receive w, [256]
  int border = 0;
  int64_t mb = 0;
  double *bd_c = nullptr, *bd_z = nullptr, *bd_l = nullptr, *bd_part = nullptr, *bd_t = nullptr;
  int bd_grid = 1;
  hipEvent_t evS0 = nullptr, evS1 = nullptr;  // around the border's share of a factorisation (last_border_ms)
  // long columns (fpsq_band_create_bordered_cols; kernels and algebra: fpsq_band.hip.h "long columns"): `cols` columns of A are
  // kept out of the band.  bc_c / bc_z hold U and Z = B^-1 U, bc_l the factor of S, bc_part the partials; vrows = 16 bc_grid
  // virtual rows lie behind row mpad of r2, r16, bd_keep and blk_keep.  t_nnz: entries of the transposed structure (a long
  // column has bc_grid of them, of value vals[nnz] = 1).  lc_*: the entries of the long columns, column by column (stored
  // row, stored entry).  bd_keep: the `keep` operand of an evaluation, resp. the x of a transposed product, [mpad + vrows].
  // bc_t[256]: (largest / smallest pivot of S)^2.  fb_*: the CSR of A_b alone for k_band_form (form_gen = 1), fb_perm its
  // entries among the stored ones
  int cols = 0;
  int64_t t_nnz = 0, fb_nnz = 0;
  int32_t *lc_ptr = nullptr, *lc_row = nullptr, *lc_ent = nullptr;
  double* bd_keep = nullptr;
  int32_t *fb_rowptr = nullptr, *fb_colind = nullptr, *fb_perm = nullptr;
  double* fb_vals = nullptr;
  // the long columns' own set, so that a handle can carry both kinds (the rows keep bd_*): bc_c / bc_z: U and Z_c, [mpad][16];
  // bc_l: the factor of S_c; bc_part: [bc_grid][256]; bc_t: [256] unused slots of a reduction, then the pivot ratio; bc_grid:
  // workgroups of the columns' reductions, over all m rows (vrows = 16 bc_grid); lc_cols: the long columns, ascending.  ARROW
  // (fpsq_band_create_arrow, border > 0 and cols > 0; fpsq_band.hip.h "arrow band"): bc_g: G = U_s' - U_b'Z_r, [16][16];
  // behind bc_part's [bc_grid][256] the rows' partials of the fused reduction, [bd_grid][256]; arrow_fused: FPSQ_ARROW_FUSED (default 1)
  double *bc_c = nullptr, *bc_z = nullptr, *bc_l = nullptr, *bc_part = nullptr, *bc_t = nullptr, *bc_g = nullptr;
  int bc_grid = 1;
  int32_t* lc_cols = nullptr;
  bool arrow_fused = true;
  // counts the numeric factorisations of this handle, whoever asked for them: a model that depends on the values a
  // factorisation left in vals / t_vals (fpsq_band_nlp_*) remembers the count it saw
  uint64_t fact_gen = 0;
  fpsq_band_info info{};
};

// fpsq_band_qp_create: the model's vectors on the handle's device and what an evaluation needs besides the handle's own
// buffers (which it borrows: in_a / in_b / o_p1 / o_p2 / o_q1 stage host-resident arguments, xn holds the packed
// right-hand sides of the A product, o_q2 keeps c resp. A v between the two product kernels)
struct fpsq_band_qp_s {
  fpsq_band b = nullptr;
  double *q = nullptr, *d = nullptr, *bp = nullptr;  // n, n, m (b in the STORED row order)
  double *partP = nullptr, *partE = nullptr;         // per-workgroup partial sums of the two product kernels, [grid][2]
  int lgA = 1, lgT = 1;                              // lanes per row of A / of A' (lane_group)
  int gridP = 1, gridE = 1;
  bool gather_g = false;  // FPSQ_BAND_QP_G=1: g formed at gather time instead of by k_bq_pack (A/B runs)
  // fpsq_band_qp_create_csr: Q = diag(q) + R.  R = the off-diagonal part as full-row CSR (both triangles), tv = the n-vector
  // the A' epilogue leaves p2 resp. Ptv in for the launch that subtracts R tv, partF = k_bq_pack_sq's partials of f, [gridR]
  bool sparse_q = false;
  int32_t *r_rowptr = nullptr, *r_colind = nullptr;
  double *r_vals = nullptr, *tv = nullptr, *partF = nullptr;
  int lgR = 1, gridR = 1;  // lanes per row of R (lane_group)
  // rows of R listed apart from the CSR above (fpsq_band.hip.h "LONG ROWS"; fpsq_band_nlp_create_coupled_arrow alone sets it)
  const fpsq::bq_long_rows* long_rows = nullptr;
  std::vector<void*> allocs;  // every device buffer above: freed by fpsq_band_qp_destroy
};

namespace {
thread_local std::string g_band_create_error;

// Reverse Cuthill-McKee on the rows of A (two rows adjacent when they share a column: the graph of A A').  Returns the new
// order (position -> caller's row) or an empty vector when the adjacency is too large to walk (sum over the columns of
// length^2 > 4e8).  Start nodes: minimum degree, moved to a pseudo-peripheral node by two breadth-first sweeps.
std::vector<int32_t> rcm_rows(int64_t m, int64_t n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci) {
  std::vector<int32_t> cp(n + 1, 0);
  for (int64_t i = 0; i < m; ++i)
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) cp[ci[k] + 1]++;
  double work = 0.0;
  for (int64_t c = 0; c < n; ++c) {
    work += (double)cp[c + 1] * cp[c + 1];
    cp[c + 1] += cp[c];
  }
  if (work > 4e8) return {};
  std::vector<int32_t> cr(std::max<int64_t>(rp[m], 1)), nxt(cp.begin(), cp.end() - 1);
  for (int64_t i = 0; i < m; ++i)
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) cr[nxt[ci[k]]++] = (int32_t)i;
  std::vector<int64_t> deg(m, 0);
  for (int64_t i = 0; i < m; ++i)
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) deg[i] += cp[ci[k] + 1] - cp[ci[k]] - 1;
  std::vector<int32_t> order;
  order.reserve(m);
  std::vector<int32_t> mark(m, -1);  // mark[i] = id of the sweep that reached row i
  std::vector<char> placed(m, 0);
  std::vector<int32_t> level, nbr;
  int sweep = 0;
  // breadth-first sweep from `root` over the not yet placed rows; returns the visiting order (neighbours by degree)
  auto bfs = [&](int32_t root, std::vector<int32_t>& out) {
    out.clear();
    ++sweep;
    mark[root] = sweep;
    out.push_back(root);
    for (size_t h = 0; h < out.size(); ++h) {
      const int32_t u = out[h];
      nbr.clear();
      for (int32_t k = rp[u]; k < rp[u + 1]; ++k)
        for (int32_t t = cp[ci[k]]; t < cp[ci[k] + 1]; ++t) {
          const int32_t v = cr[t];
          if (!placed[v] && mark[v] != sweep) {
            mark[v] = sweep;
            nbr.push_back(v);
          }
        }
      std::sort(nbr.begin(), nbr.end(), [&](int32_t a, int32_t b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; });
      out.insert(out.end(), nbr.begin(), nbr.end());
    }
  };
  std::vector<int32_t> byd(m);
  for (int64_t i = 0; i < m; ++i) byd[i] = (int32_t)i;
  std::sort(byd.begin(), byd.end(), [&](int32_t a, int32_t b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; });
  size_t cursor = 0;
  while ((int64_t)order.size() < m) {
    while (placed[byd[cursor]]) ++cursor;
    int32_t root = byd[cursor];
    for (int pass = 0; pass < 2; ++pass) {  // towards a pseudo-peripheral node: restart from the last node reached
      bfs(root, level);
      root = level.back();
    }
    bfs(root, level);
    for (int32_t v : level) placed[v] = 1;
    order.insert(order.end(), level.begin(), level.end());
  }
  std::reverse(order.begin(), order.end());
  return order;
}

// The ordering part of the symbolic phase, host only (also behind fpsq_band_analyze, which needs no device): validates
// the pattern, reorders the rows when that pays (rp / ci are replaced by the reordered structure; rperm_h / vperm_h map
// stored rows / entries to the caller's, empty = identity) and decides on the two elimination chains.  Returns an error
// text, empty on success.
std::string band_order_rows(int64_t n, int64_t m, std::vector<int32_t>& rp, std::vector<int32_t>& ci,
                            std::vector<int32_t>& rperm_h, std::vector<int32_t>& vperm_h, int& chain_safe, int& chain_bw) {
  const int64_t nnz = rp[m];
  chain_safe = chain_bw = 0;
  // validate, then the natural half bandwidth (rows): if the band is wide, try a reverse Cuthill-McKee ordering of the rows
  // (LDLFactorizations' ldl_analyze computes a fill-reducing ordering at this point; for a band factorisation the
  // ordering to look for is the bandwidth-reducing one).  FPSQ_BAND_REORDER = 0 never, 1 always tries.
  for (int64_t i = 0; i < m; ++i) {
    if (rp[i + 1] < rp[i] || rp[i + 1] > nnz) {
      return "fpsq_band_create: rowptr not monotone";
    }
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k)
      if (ci[k] < 0 || ci[k] >= n) {
        return "fpsq_band_create: column index out of range";
      }
  }
  {
    auto bandwidth_rows = [&](const std::vector<int32_t>& pos) {  // pos[row] = position; empty = identity
      std::vector<int32_t> lo(n, INT32_MAX), hi(n, -1);
      for (int64_t i = 0; i < m; ++i) {
        const int32_t p = pos.empty() ? (int32_t)i : pos[i];
        for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
          lo[ci[k]] = std::min(lo[ci[k]], p);
          hi[ci[k]] = std::max(hi[ci[k]], p);
        }
      }
      int64_t w = 0;
      for (int64_t c = 0; c < n; ++c)
        if (hi[c] >= 0) w = std::max<int64_t>(w, hi[c] - lo[c]);
      return w;
    };
    // row `ord[p]` of the current structure becomes row p; the maps to the caller's numbering are composed
    auto apply_order = [&](const std::vector<int32_t>& ord) {
      std::vector<int32_t> rp2(m + 1, 0), ci2(std::max<int64_t>(nnz, 1)), vp2(std::max<int64_t>(nnz, 1)), rr2(m);
      for (int64_t p = 0; p < m; ++p) {
        const int32_t r = ord[p];
        rr2[p] = rperm_h.empty() ? r : rperm_h[r];
        rp2[p + 1] = rp2[p] + (rp[r + 1] - rp[r]);
        for (int32_t k = rp[r], t = rp2[p]; k < rp[r + 1]; ++k, ++t) {
          ci2[t] = ci[k];
          vp2[t] = vperm_h.empty() ? k : vperm_h[k];
        }
      }
      rp.swap(rp2);
      ci.swap(ci2);
      rperm_h.swap(rr2);
      vperm_h.swap(vp2);
    };
    int mode = -1;  // auto
    if (const char* ev = std::getenv("FPSQ_BAND_REORDER")) mode = std::atoi(ev);
    const int64_t nbk = (m + kDB - 1) / kDB;
    int64_t bw_rows = bandwidth_rows({});
    if (mode != 0 && (mode == 1 || bw_rows / kDB > std::max<int64_t>(nbk / 8, 2))) {
      std::vector<int32_t> ord = rcm_rows(m, n, rp, ci);
      if (!ord.empty()) {
        std::vector<int32_t> pos(m);
        for (int64_t p = 0; p < m; ++p) pos[ord[p]] = (int32_t)p;
        const int64_t bw_new = bandwidth_rows(pos);
        if (bw_new / kDB < bw_rows / kDB) {  // fewer blocks in the band: take it
          apply_order(ord);
          bw_rows = bw_new;
        }
      }
    }
    // TWO ELIMINATION CHAINS.  A banded Cholesky is a chain of m / 128 dependent block steps, each a few latency-bound
    // launches.  Ordering the blocks from BOTH ends towards the middle -- stored block 2 c = block c from the top, stored
    // block 2 c + 1 = the c-th block of 128 rows from the bottom (rows descending) -- keeps the matrix banded (twice as
    // wide) and makes the even and the odd blocks two independent chains until they meet: their steps run side by side
    // on two streams, the chain is half as long.  Only the last 2 (chain_bw + 1) blocks and the rows left in the middle
    // are eliminated one after the other.  FPSQ_BAND_TWOCHAIN=0 turns it off.
    int two = 1;
    if (const char* ev = std::getenv("FPSQ_BAND_TWOCHAIN")) two = std::atoi(ev);
    const int64_t C = m / (2 * kDB);
    const int64_t bwc = (bw_rows + kDB - 1) / kDB;  // block distance two coupled rows of one chain can have
    if (two && bwc >= 1 && C - bwc - 1 >= 4 * (bwc + 1)) {
      std::vector<int32_t> ord(m);
      int64_t p = 0;
      for (int64_t c = 0; c < C; ++c) {
        for (int64_t t = 0; t < kDB; ++t) ord[p++] = (int32_t)(c * kDB + t);
        for (int64_t t = 0; t < kDB; ++t) ord[p++] = (int32_t)(m - 1 - c * kDB - t);
      }
      for (int64_t r = C * kDB; r < m - C * kDB; ++r) ord[p++] = (int32_t)r;
      apply_order(ord);
      chain_safe = (int)(C - bwc - 1);
      chain_bw = (int)bwc;
    }
  }
  return std::string();
}

// half bandwidth of A A' in 128-row blocks over the first `rows` rows of a stored structure
int64_t band_blocks(int64_t n, int64_t rows, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci) {
  std::vector<int32_t> lo(n, INT32_MAX), hi(n, -1);
  for (int64_t i = 0; i < rows; ++i)
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
      lo[ci[k]] = std::min(lo[ci[k]], (int32_t)(i / kDB));
      hi[ci[k]] = std::max(hi[ci[k]], (int32_t)(i / kDB));
    }
  int64_t bwb = 0;
  for (int64_t c = 0; c < n; ++c)
    if (hi[c] >= 0) bwb = std::max<int64_t>(bwb, hi[c] - lo[c]);
  return bwb;
}

// The ordering with a BORDER of at most max_border rows (include/fpsq.h, fpsq_band_create_bordered, has the rule): first the
// ordering of all rows, as band_order_rows leaves it; then, candidates being the max_border rows of widest column span
// (ties: the lower row first), the shortest prefix of them whose removal leaves rows that band_order_rows orders into a band
// at most a quarter as wide (in blocks).  If there is one, those rows are stored last (ascending) behind that ordering of
// the others and `border` counts them; else the result is the ordering of all rows and border = 0.
std::string band_order(int64_t n, int64_t m, std::vector<int32_t>& rp, std::vector<int32_t>& ci, std::vector<int32_t>& rperm_h,
                       std::vector<int32_t>& vperm_h, int& chain_safe, int& chain_bw, int max_border, int& border) {
  border = 0;
  std::vector<int32_t> rp0, ci0;
  if (max_border > 0) {
    rp0 = rp;
    ci0 = ci;
  }
  const std::string msg = band_order_rows(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw);
  if (!msg.empty() || max_border <= 0 || m < 2) return msg;
  const int64_t bwb0 = band_blocks(n, m, rp, ci);
  if (bwb0 == 0) return msg;
  std::vector<int64_t> span(m, 0);
  for (int64_t i = 0; i < m; ++i) {
    int32_t lo = INT32_MAX, hi = -1;
    for (int32_t k = rp0[i]; k < rp0[i + 1]; ++k) {
      lo = std::min(lo, ci0[k]);
      hi = std::max(hi, ci0[k]);
    }
    span[i] = hi >= 0 ? (int64_t)hi - lo + 1 : 0;
  }
  std::vector<int32_t> cand(m);
  for (int64_t i = 0; i < m; ++i) cand[i] = (int32_t)i;
  const int64_t ncand = std::min<int64_t>(max_border, m - 1);
  std::partial_sort(cand.begin(), cand.begin() + ncand, cand.end(),
                    [&](int32_t a, int32_t b) { return span[a] != span[b] ? span[a] > span[b] : a < b; });
  std::vector<char> out(m, 0);
  for (int64_t k = 1; k <= ncand; ++k) {
    out[cand[k - 1]] = 1;
    const int64_t mb = m - k;
    std::vector<int32_t> rows_b, rp_b(1, 0), ci_b, ent_b;  // the other rows in the caller's order; ent_b: entry -> the caller's
    rows_b.reserve(mb);
    for (int64_t i = 0; i < m; ++i) {
      if (out[i]) continue;
      rows_b.push_back((int32_t)i);
      for (int32_t t = rp0[i]; t < rp0[i + 1]; ++t) {
        ci_b.push_back(ci0[t]);
        ent_b.push_back(t);
      }
      rp_b.push_back((int32_t)ci_b.size());
    }
    ci_b.resize(std::max<size_t>(ci_b.size(), 1));
    std::vector<int32_t> rperm_b, vperm_b;
    int cs = 0, cb = 0;
    if (!band_order_rows(n, mb, rp_b, ci_b, rperm_b, vperm_b, cs, cb).empty()) break;
    if (4 * band_blocks(n, mb, rp_b, ci_b) > bwb0) continue;
    // taken: the band rows as ordered, then the border rows
    const int64_t nnz = rp0[m], nnz_b = rp_b[mb];
    std::vector<int32_t> rp2(m + 1, 0), ci2(std::max<int64_t>(nnz, 1)), rr2(m), vp2(std::max<int64_t>(nnz, 1));
    for (int64_t p = 0; p < mb; ++p) {
      rr2[p] = rows_b[rperm_b.empty() ? p : rperm_b[p]];
      rp2[p + 1] = rp_b[p + 1];
    }
    for (int64_t t = 0; t < nnz_b; ++t) {
      ci2[t] = ci_b[t];
      vp2[t] = ent_b[vperm_b.empty() ? t : vperm_b[t]];
    }
    int64_t p = mb;
    for (int64_t i = 0; i < m; ++i) {
      if (!out[i]) continue;
      rr2[p] = (int32_t)i;
      rp2[p + 1] = rp2[p] + (rp0[i + 1] - rp0[i]);
      for (int32_t t = rp0[i], u = rp2[p]; t < rp0[i + 1]; ++t, ++u) {
        ci2[u] = ci0[t];
        vp2[u] = t;
      }
      ++p;
    }
    rp.swap(rp2);
    ci.swap(ci2);
    rperm_h.swap(rr2);
    vperm_h.swap(vp2);
    chain_safe = cs;
    chain_bw = cb;
    border = (int)k;
    break;
  }
  return msg;
}

// The ordering with at most max_cols LONG COLUMNS taken out (include/fpsq.h, "LONG COLUMNS", has the rule): first the ordering
// of the rows on all columns, as band_order_rows leaves it; then, candidates being the max_cols columns with the most entries
// (ties: the lower column first), the shortest prefix of them after whose removal no row is empty and band_order_rows orders
// the rows into a band at most a quarter as wide (in blocks).  If there is one, the result is THAT ordering of the rows, every
// row with all its entries (the long columns' included, columns are not renumbered), and lcols lists the columns ascending;
// else the result is the ordering on all columns and lcols is empty.
std::string band_order_cols(int64_t n, int64_t m, std::vector<int32_t>& rp, std::vector<int32_t>& ci,
                            std::vector<int32_t>& rperm_h, std::vector<int32_t>& vperm_h, int& chain_safe, int& chain_bw,
                            int max_cols, std::vector<int32_t>& lcols) {
  lcols.clear();
  const std::vector<int32_t> rp0 = rp, ci0 = ci;
  const std::string msg = band_order_rows(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw);
  if (!msg.empty() || max_cols <= 0 || m < 2 || n < 2) return msg;
  const int64_t bwb0 = band_blocks(n, m, rp, ci);
  if (bwb0 == 0) return msg;
  const int64_t nnz = rp0[m];
  std::vector<int64_t> cnt(n, 0);
  for (int64_t k = 0; k < nnz; ++k) cnt[ci0[k]]++;
  std::vector<int32_t> cand(n);
  for (int64_t c = 0; c < n; ++c) cand[c] = (int32_t)c;
  const int64_t ncand = std::min<int64_t>(max_cols, n - 1);
  std::partial_sort(cand.begin(), cand.begin() + ncand, cand.end(),
                    [&](int32_t a, int32_t b) { return cnt[a] != cnt[b] ? cnt[a] > cnt[b] : a < b; });
  std::vector<char> out(n, 0);
  for (int64_t k = 1; k <= ncand; ++k) {
    out[cand[k - 1]] = 1;
    std::vector<int32_t> rp_b(1, 0), ci_b;  // the rows on the remaining columns, in the caller's order
    bool empty_row = false;
    for (int64_t i = 0; i < m && !empty_row; ++i) {
      for (int32_t t = rp0[i]; t < rp0[i + 1]; ++t)
        if (!out[ci0[t]]) ci_b.push_back(ci0[t]);
      empty_row = (int32_t)ci_b.size() == rp_b.back();
      rp_b.push_back((int32_t)ci_b.size());
    }
    if (empty_row) break;  // rule (a); a longer prefix empties the same row
    ci_b.resize(std::max<size_t>(ci_b.size(), 1));
    std::vector<int32_t> rperm_b, vperm_b;
    int cs = 0, cb = 0;
    if (!band_order_rows(n, m, rp_b, ci_b, rperm_b, vperm_b, cs, cb).empty()) break;
    if (4 * band_blocks(n, m, rp_b, ci_b) > bwb0) continue;
    // taken: the rows in that order, each with all its entries
    if (rperm_b.empty()) {
      rp = rp0;
      ci = ci0;
      rperm_h.clear();
      vperm_h.clear();
    } else {
      std::vector<int32_t> rp2(m + 1, 0), ci2(std::max<int64_t>(nnz, 1)), vp2(std::max<int64_t>(nnz, 1));
      for (int64_t p = 0; p < m; ++p) {
        const int32_t r = rperm_b[p];
        rp2[p + 1] = rp2[p] + (rp0[r + 1] - rp0[r]);
        for (int32_t t = rp0[r], u = rp2[p]; t < rp0[r + 1]; ++t, ++u) {
          ci2[u] = ci0[t];
          vp2[u] = t;
        }
      }
      rp.swap(rp2);
      ci.swap(ci2);
      rperm_h.swap(rperm_b);
      vperm_h.swap(vp2);
    }
    chain_safe = cs;
    chain_bw = cb;
    lcols.assign(cand.begin(), cand.begin() + k);
    std::sort(lcols.begin(), lcols.end());
    break;
  }
  return msg;
}

// The ordering of an ARROW handle: at most max_border border rows AND at most max_cols long columns (include/fpsq.h, "ARROW
// BAND", has the rule).  1: Cc = the max_cols columns with the most entries, Rc = the max_border rows of widest span over the
// columns not in Cc.  2: the column rule on the rows not in Rc (baseline and trials), rule (a) over all rows: L.  3: the row
// rule on the columns not in L: R.  4: L empty -> band_order, R empty -> band_order_cols, either maximum 0 -> the other rule.
// Both taken: the band rows as step 3 ordered them, every row with all its entries, then the rows of R ascending.
std::string band_order_arrow(int64_t n, int64_t m, std::vector<int32_t>& rp, std::vector<int32_t>& ci,
                             std::vector<int32_t>& rperm_h, std::vector<int32_t>& vperm_h, int& chain_safe, int& chain_bw,
                             int max_border, int max_cols, int& border, std::vector<int32_t>& lcols) {
  border = 0;
  lcols.clear();
  if (max_cols <= 0) return band_order(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw, max_border, border);
  if (max_border <= 0) return band_order_cols(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw, max_cols, lcols);
  const int64_t nnz = rp[m];
  bool valid = m >= 2 && n >= 2;
  for (int64_t i = 0; i < m && valid; ++i) {
    valid = rp[i + 1] >= rp[i] && rp[i + 1] <= nnz;
    for (int32_t k = rp[i]; valid && k < rp[i + 1]; ++k) valid = ci[k] >= 0 && ci[k] < n;
  }
  if (!valid)  // (band_order reports a bad pattern; with fewer than two rows or columns no column is taken)
    return band_order(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw, max_border, border);
  const std::vector<int32_t> rp0 = rp, ci0 = ci;
  // the rows not in skip_row (null: all rows) on the columns not in drop_col, in the caller's order: CSR, the rows' and the
  // entries' numbers among the caller's
  struct Sub { std::vector<int32_t> rows, rp, ci, ent; };
  auto sub_pattern = [&](const std::vector<char>* skip_row, const std::vector<char>& drop_col) {
    Sub u;
    u.rp.assign(1, 0);
    for (int64_t i = 0; i < m; ++i) {
      if (skip_row && (*skip_row)[i]) continue;
      u.rows.push_back((int32_t)i);
      for (int32_t t = rp0[i]; t < rp0[i + 1]; ++t)
        if (!drop_col[ci0[t]]) {
          u.ci.push_back(ci0[t]);
          u.ent.push_back(t);
        }
      u.rp.push_back((int32_t)u.ci.size());
    }
    u.ci.resize(std::max<size_t>(u.ci.size(), 1));
    return u;
  };
  // band_order_rows on such a pattern: the half bandwidth in blocks, -1 when the ordering fails
  auto ordered_blocks = [&](Sub& u, std::vector<int32_t>& rperm_b, int& cs, int& cb) -> int64_t {
    std::vector<int32_t> vperm_b;
    rperm_b.clear();
    const int64_t rows = (int64_t)u.rows.size();
    if (!band_order_rows(n, rows, u.rp, u.ci, rperm_b, vperm_b, cs, cb).empty()) return -1;
    return band_blocks(n, rows, u.rp, u.ci);
  };
  // 1: the candidates
  std::vector<int64_t> cnt(n, 0);
  for (int64_t k = 0; k < nnz; ++k) cnt[ci0[k]]++;
  std::vector<int32_t> ccand(n);
  for (int64_t c = 0; c < n; ++c) ccand[c] = (int32_t)c;
  const int64_t nccand = std::min<int64_t>(max_cols, n - 1);
  std::partial_sort(ccand.begin(), ccand.begin() + nccand, ccand.end(),
                    [&](int32_t a, int32_t b) { return cnt[a] != cnt[b] ? cnt[a] > cnt[b] : a < b; });
  std::vector<char> in_cc(n, 0);
  for (int64_t k = 0; k < nccand; ++k) in_cc[ccand[k]] = 1;
  // the max_border rows of widest span over the columns without `drop`, widest first
  auto row_candidates = [&](const std::vector<char>& drop, std::vector<int32_t>& cand) {
    std::vector<int64_t> span(m, 0);
    for (int64_t i = 0; i < m; ++i) {
      int32_t lo = INT32_MAX, hi = -1;
      for (int32_t k = rp0[i]; k < rp0[i + 1]; ++k) {
        if (drop[ci0[k]]) continue;
        lo = std::min(lo, ci0[k]);
        hi = std::max(hi, ci0[k]);
      }
      span[i] = hi >= 0 ? (int64_t)hi - lo + 1 : 0;
    }
    cand.resize(m);
    for (int64_t i = 0; i < m; ++i) cand[i] = (int32_t)i;
    const int64_t nc = std::min<int64_t>(max_border, m - 1);
    std::partial_sort(cand.begin(), cand.begin() + nc, cand.end(),
                      [&](int32_t a, int32_t b) { return span[a] != span[b] ? span[a] > span[b] : a < b; });
    cand.resize(nc);
  };
  std::vector<int32_t> rcand;
  row_candidates(in_cc, rcand);
  std::vector<char> in_rc(m, 0);
  for (int32_t r : rcand) in_rc[r] = 1;
  // 2: the columns, on the rows not in Rc
  std::vector<char> is_l(n, 0);
  int nl = 0;
  {
    std::vector<int32_t> rperm_b;
    int cs = 0, cb = 0;
    Sub base = sub_pattern(&in_rc, is_l);
    const int64_t bwb0 = ordered_blocks(base, rperm_b, cs, cb);
    std::vector<char> out(n, 0);
    for (int64_t k = 1; bwb0 > 0 && k <= nccand; ++k) {
      out[ccand[k - 1]] = 1;
      bool empty_row = false;  // rule (a), over ALL rows
      for (int64_t i = 0; i < m && !empty_row; ++i) {
        bool any = false;
        for (int32_t t = rp0[i]; t < rp0[i + 1] && !any; ++t) any = !out[ci0[t]];
        empty_row = !any;
      }
      if (empty_row) break;
      Sub trial = sub_pattern(&in_rc, out);
      const int64_t bw = ordered_blocks(trial, rperm_b, cs, cb);
      if (bw < 0) break;
      if (4 * bw > bwb0) continue;
      is_l = out;
      nl = (int)k;
      break;
    }
  }
  auto restore = [&] {
    rp = rp0;
    ci = ci0;
    rperm_h.clear();
    vperm_h.clear();
  };
  if (nl == 0) {  // 4: no long columns: the row border's rule alone
    restore();
    return band_order(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw, max_border, border);
  }
  // 3: the rows, on the columns not in L
  int nr = 0, cs_t = 0, cb_t = 0;
  std::vector<char> in_r(m, 0);
  std::vector<int32_t> rows_t, rperm_t;
  {
    std::vector<int32_t> rperm_b;
    int cs = 0, cb = 0;
    Sub base = sub_pattern(nullptr, is_l);
    const int64_t bwb0 = ordered_blocks(base, rperm_b, cs, cb);
    row_candidates(is_l, rcand);
    std::vector<char> out(m, 0);
    for (int64_t k = 1; bwb0 > 0 && k <= (int64_t)rcand.size(); ++k) {
      out[rcand[k - 1]] = 1;
      Sub trial = sub_pattern(&out, is_l);
      const int64_t bw = ordered_blocks(trial, rperm_b, cs, cb);
      if (bw < 0) break;
      if (4 * bw > bwb0) continue;
      in_r = out;
      nr = (int)k;
      rows_t.swap(trial.rows);
      rperm_t.swap(rperm_b);
      cs_t = cs;
      cb_t = cb;
      break;
    }
  }
  if (nr == 0) {  // 4: no border rows: the column rule alone, decided again on all rows
    restore();
    return band_order_cols(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw, max_cols, lcols);
  }
  // both: the band rows in the order of step 3, then the border rows ascending, every row with all its entries
  const int64_t mb = m - nr;
  std::vector<int32_t> rp2(m + 1, 0), ci2(std::max<int64_t>(nnz, 1)), rr2(m), vp2(std::max<int64_t>(nnz, 1));
  int64_t p = 0;
  auto put_row = [&](int32_t r) {
    rr2[p] = r;
    rp2[p + 1] = rp2[p] + (rp0[r + 1] - rp0[r]);
    for (int32_t t = rp0[r], u = rp2[p]; t < rp0[r + 1]; ++t, ++u) {
      ci2[u] = ci0[t];
      vp2[u] = t;
    }
    ++p;
  };
  for (int64_t q = 0; q < mb; ++q) put_row(rows_t[rperm_t.empty() ? q : rperm_t[q]]);
  for (int64_t i = 0; i < m; ++i)
    if (in_r[i]) put_row((int32_t)i);
  bool identity = true;  // (the border rows already last and the band rows kept in place: not a reordered handle)
  for (int64_t q = 0; q < m && identity; ++q) identity = rr2[q] == (int32_t)q;
  rp.swap(rp2);
  ci.swap(ci2);
  rperm_h.swap(rr2);
  vperm_h.swap(vp2);
  if (identity) {
    rperm_h.clear();
    vperm_h.clear();
  }
  chain_safe = cs_t;
  chain_bw = cb_t;
  border = nr;
  for (int64_t c = 0; c < n; ++c)
    if (is_l[c]) lcols.push_back((int32_t)c);
  return std::string();
}

inline size_t blk_off(const fpsq_band b, int64_t i, int64_t j) {  // block (i, j), i - (band_w - 1) <= j <= i
  return ((size_t)i * b->band_w + (size_t)(j - i + b->band_w - 1)) * kDB * kDB;
}

// The correction of an M-solve on a bordered handle, behind the sweeps (y: b->r2 with NC = 2, b->r16 with NC = 16): rows < mb
// hold B^-1 r, rows mb .. m - 1 still the border's right-hand side t; afterwards all of them hold M^-1 [r; t]
template <int NC>
void border_correct(fpsq_band b, double* y) {
  hipLaunchKernelGGL(k_border_reduce<NC>, dim3(b->bd_grid), dim3(256), 0, b->stream, b->bd_c, y, (int)b->mb, b->border,
                     b->bd_part, b->bd_t);
  hipLaunchKernelGGL(k_border_update<NC>, dim3(b->bd_grid), dim3(256), 0, b->stream, b->bd_z, b->bd_l, b->bd_part, b->bd_grid,
                     b->bd_t, y, (int)b->mb, b->border);
}

// The correction of an M-solve on a handle with long columns, behind the sweeps (y as above): all rows hold B^-1 r; afterwards
// they hold M^-1 r = y - Z w and the virtual rows behind row mpad hold w = U'(y - Z w)
template <int NC>
void cols_correct(fpsq_band b, double* y) {
  hipLaunchKernelGGL(k_border_reduce<NC>, dim3(b->bc_grid), dim3(256), 0, b->stream, b->bc_c, y, (int)b->m, 0, b->bc_part,
                     b->bc_t);
  hipLaunchKernelGGL(k_cols_update<NC>, dim3(b->bc_grid), dim3(256), 0, b->stream, b->bc_z, b->bc_l, b->bc_part, b->bc_grid, y,
                     (int)b->m, (int)b->mpad);
}

// The correction of an M-solve on an ARROW handle (border rows and long columns), behind the sweeps (y as above): the fused
// pair of fpsq_band.hip.h "arrow band", or with FPSQ_ARROW_FUSED=0 the two corrections above one after the other.  The fused
// reduction runs on the rows' grid (band rows), the update on the columns' grid (all rows and the virtual rows); the rows'
// partials of the fused form lie behind the columns' in bc_part
template <int NC>
void arrow_correct(fpsq_band b, double* y) {
  if (!b->arrow_fused) {
    border_correct<NC>(b, y);
    cols_correct<NC>(b, y);
    return;
  }
  double* part_r = b->bc_part + (size_t)b->bc_grid * 256;
  hipLaunchKernelGGL(k_arrow_reduce<NC>, dim3(b->bd_grid), dim3(256), 0, b->stream, b->bd_c, b->bc_c, y, (int)b->mb, b->border,
                     part_r, b->bc_part, b->bd_t);
  hipLaunchKernelGGL(k_arrow_update<NC>, dim3(b->bc_grid), dim3(256), 0, b->stream, b->bd_z, b->bd_l, b->bc_z, b->bc_l, b->bc_g,
                     part_r, b->bc_part, b->bd_grid, b->bd_t, y, (int)b->mb, (int)b->m, (int)b->mpad);
}

// whichever correction the handle's kind asks for
template <int NC>
void band_correct(fpsq_band b, double* y) {
  if (b->border && b->cols) return arrow_correct<NC>(b, y);
  if (b->border) border_correct<NC>(b, y);
  if (b->cols) cols_correct<NC>(b, y);
}

// the chunk sums of U'keep into the virtual rows of an operand the A' kernels read beside the solutions (keep: [mpad + vrows][NC])
template <int NC>
void cols_keep(fpsq_band b, double* keep) {
  hipLaunchKernelGGL(k_border_reduce<NC>, dim3(b->bc_grid), dim3(256), 0, b->stream, b->bc_c, keep, (int)b->m, 0,
                     keep + (size_t)b->mpad * NC, b->bc_t);
}

void band_sweeps(fpsq_band b);

// q (in b->r2, [mpad][2]) <- M^-1 r2 with the banded factor (and the border's correction, whichever form the sweeps take);
// result in b->r2
void band_solve(fpsq_band b) {
  band_sweeps(b);
  band_correct<2>(b, b->r2);
}

// the sweeps on the band rows: b->r2 <- B^-1 b->r2 (rows beyond the band's blocks are not touched)
void band_sweeps(fpsq_band b) {
  hipStream_t s = b->stream;
  const int nb = (int)b->nb, bw = b->band_w - 1;
  if (b->chain)  // (both elimination chains advance side by side inside the one launch)
    return chain_sweeps(b, b->Mb, kDB, b->band_w, b->chain_safe, b->chain_bw);
  {
    int k0 = 0;
    const int cs = b->chain_safe, cb = b->chain_bw;
    hipStream_t s2 = b->stream2;
    if (cs > 0) {  // forward: the two chains side by side (each touches the blocks of its own parity only), then the rest
      hipEventRecord(b->evA, s);
      hipStreamWaitEvent(s2, b->evA, 0);
      for (int c = 0; c < cs; ++c) {
        hipLaunchKernelGGL(k_trsv_step3<true>, dim3(cb + 1), dim3(256), 0, s, b->Mb, kDB, b->invs, b->invsT, b->r2, b->y2, 2 * c,
                           b->band_w, 2);
        hipLaunchKernelGGL(k_trsv_step3<true>, dim3(cb + 1), dim3(256), 0, s2, b->Mb, kDB, b->invs, b->invsT, b->r2, b->y2,
                           2 * c + 1, b->band_w, 2);
      }
      hipEventRecord(b->evB, s2);
      hipStreamWaitEvent(s, b->evB, 0);
      k0 = 2 * cs;
    }
    for (int k = k0; k < nb; ++k)
      hipLaunchKernelGGL(k_trsv_step3<true>, dim3(std::min(bw, nb - 1 - k) + 1), dim3(256), 0, s, b->Mb, kDB, b->invs,
                         b->invsT, b->r2, b->y2, k, b->band_w, 1);
    for (int k = nb - 1; k >= k0; --k)
      hipLaunchKernelGGL(k_trsv_step3<false>, dim3(std::min(bw, k) + 1), dim3(256), 0, s, b->Mb, kDB, b->invs, b->invsT,
                         b->y2, b->r2, k, b->band_w, 1);
    if (cs > 0) {
      hipEventRecord(b->evA, s);
      hipStreamWaitEvent(s2, b->evA, 0);
      for (int c = cs - 1; c >= 0; --c) {
        hipLaunchKernelGGL(k_trsv_step3<false>, dim3(std::min(cb, c) + 1), dim3(256), 0, s, b->Mb, kDB, b->invs, b->invsT,
                           b->y2, b->r2, 2 * c, b->band_w, 2);
        hipLaunchKernelGGL(k_trsv_step3<false>, dim3(std::min(cb, c) + 1), dim3(256), 0, s2, b->Mb, kDB, b->invs, b->invsT,
                           b->y2, b->r2, 2 * c + 1, b->band_w, 2);
      }
      hipEventRecord(b->evB, s2);
      hipStreamWaitEvent(s, b->evB, 0);
    }
  }
}

// shared tail of the two solve entry points: right-hand sides of the M-solves are in b->r2
int band_finish(fpsq_band b, const double* a1, double* p1, double* q1, double* p2, double* q2) {
  hipStream_t s = b->stream;
  band_solve(b);
  // P = [a0, a1] - A' Q
  hipLaunchKernelGGL(k_csr_mv2, grid256(b->n), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals,
                     b->r2, b->atq, (int)b->n);
  hipLaunchKernelGGL(k_band_finish, grid256(b->n), dim3(256), 0, s, b->atq, b->in_a, a1, b->o_p1,
                     b->o_p2, (int)b->n);
  if (b->reordered)  // back to the caller's row order
    hipLaunchKernelGGL(k_unpack2_scatter, grid256(b->m), dim3(256), 0, s, b->r2, b->rperm, b->o_q1,
                       b->o_q2, (int)b->m);
  else
    hipLaunchKernelGGL(k_dense_unpack2, grid256(b->m), dim3(256), 0, s, b->r2, b->o_q1, b->o_q2,
                       (int)b->m);
  return solve_end(b, p1, q1, p2, q2, &b->info.last_solve_ms);
}

// ---- the phases of fpsq_band_create, in the order it runs them

// What the host phase leaves for the others: the stored (reordered) structure and its transpose
struct BandSymbolic {
  std::vector<int32_t> rp, ci;        // the stored CSR
  std::vector<int32_t> rperm, vperm;  // stored row / entry -> the caller's (empty: identity)
  std::vector<int32_t> tptr, trow, tperm;  // the transposed structure (for P = rhs - A' Q) with the value permutation
  std::vector<int2> span;                  // {first, last column} of every row
  int maxspan = 1, chain_safe = 0, chain_bw = 0;  // (maxspan: over the band rows)
  int64_t bwb = 0;  // half bandwidth in blocks (of the band rows)
  int border = 0;   // rows stored last and eliminated as a border
  // long columns (ascending), the workgroups of their reductions, their entries column by column (stored row / entry), and
  // the CSR of the other columns alone with its entries among the stored ones (k_band_form)
  std::vector<int32_t> lcols, lc_ptr, lc_row, lc_ent, rp_b, ci_b, perm_b;
  int vgrid = 0;
  int64_t t_nnz = 0;
};

// Validate and order on the host (the role of ldl_analyze, src/solve_two_systems_struct.jl:344): the structure of
// A A' + delta I is a band whose half width is the largest row distance of two entries of one column of A.  Reads the
// caller's CSR (host or device memory); returns an error text, empty on success.
std::string band_symbolic(int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int max_border, int max_cols,
                          bool arrow, BandSymbolic& sy) {
  std::vector<int32_t>&rp = sy.rp, &ci = sy.ci;
  rp.resize(m + 1);
  if (hipMemcpy(rp.data(), rowptr, (size_t)(m + 1) * 4, hipMemcpyDefault) != hipSuccess || rp[0] != 0)
    return "fpsq_band_create: cannot read rowptr (0-based CSR expected)";
  const int64_t nnz = rp[m];
  ci.resize(std::max<int64_t>(nnz, 1));
  if (nnz > 0 && (!colind || hipMemcpy(ci.data(), colind, (size_t)nnz * 4, hipMemcpyDefault) != hipSuccess))
    return "fpsq_band_create: cannot read colind";
  for (int64_t i = 0; arrow && i < m; ++i)
    if (rp[i + 1] < rp[i] || rp[i + 1] > nnz) return "fpsq_band_create: rowptr not monotone";
  const std::string msg =
      arrow ? band_order_arrow(n, m, rp, ci, sy.rperm, sy.vperm, sy.chain_safe, sy.chain_bw, max_border, max_cols, sy.border,
                               sy.lcols)
      : max_cols > 0 ? band_order_cols(n, m, rp, ci, sy.rperm, sy.vperm, sy.chain_safe, sy.chain_bw, max_cols, sy.lcols)
                     : band_order(n, m, rp, ci, sy.rperm, sy.vperm, sy.chain_safe, sy.chain_bw, max_border, sy.border);
  if (!msg.empty()) return msg;
  const int64_t mb = m - sy.border;
  const int ncols = (int)sy.lcols.size();
  const int64_t mpad = (m + kDB - 1) / kDB * kDB;
  sy.vgrid = ncols ? (int)std::max<int64_t>(1, std::min<int64_t>((m + 255) / 256, kBorderGrid)) : 0;
  std::vector<int8_t> lidx(ncols ? n : 0, -1);  // column -> its place among the long ones
  for (int i = 0; i < ncols; ++i) lidx[sy.lcols[i]] = (int8_t)i;
  auto is_long = [&](int32_t c) { return ncols && lidx[c] >= 0; };
  std::vector<int32_t> cfirst(n, INT32_MAX), clast(n, -1), seen(n, -1);
  std::vector<int32_t>& tcnt = sy.tptr;
  tcnt.assign(n + 1, 0);
  sy.span.resize(m);
  bool has_dup = false;
  for (int64_t i = 0; i < m; ++i) {  // (band_order has validated the pattern)
    int lo = INT32_MAX, hi = -1;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
      const int32_t c = ci[k];
      has_dup |= seen[c] == (int32_t)i;
      seen[c] = (int32_t)i;
      if (is_long(c)) continue;  // (neither in a span nor in the band; its transposed entries are virtual, below)
      lo = std::min(lo, c);
      hi = std::max(hi, c);
      if (i < mb) {
        cfirst[c] = std::min<int32_t>(cfirst[c], (int32_t)i);
        clast[c] = std::max<int32_t>(clast[c], (int32_t)i);
      }
      tcnt[c + 1]++;
    }
    if (hi < 0) lo = hi = 0;
    sy.span[i] = int2{lo, hi};
    if (i < mb) sy.maxspan = std::max(sy.maxspan, hi - lo + 1);
  }
  if (has_dup) return "fpsq_band_create: the CSR pattern has duplicate entries (sum them first)";
  for (int64_t c = 0; c < n; ++c)
    if (clast[c] >= 0) sy.bwb = std::max<int64_t>(sy.bwb, clast[c] / kDB - cfirst[c] / kDB);
  for (int i = 0; i < ncols; ++i) tcnt[sy.lcols[i] + 1] = sy.vgrid;
  for (int64_t c = 0; c < n; ++c) tcnt[c + 1] += tcnt[c];
  sy.t_nnz = tcnt[n];
  sy.trow.resize(std::max<int64_t>(sy.t_nnz, 1));
  sy.tperm.resize(std::max<int64_t>(sy.t_nnz, 1));
  std::vector<int32_t> nxt(tcnt.begin(), tcnt.end() - 1);
  std::vector<std::vector<int32_t>> lrow(ncols), lent(ncols);
  if (ncols) sy.rp_b.assign(1, 0);
  for (int64_t i = 0; i < m; ++i) {
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
      if (is_long(ci[k])) {
        lrow[lidx[ci[k]]].push_back((int32_t)i);
        lent[lidx[ci[k]]].push_back(k);
        continue;
      }
      const int32_t t = nxt[ci[k]]++;
      sy.trow[t] = (int32_t)i;
      sy.tperm[t] = k;
      if (ncols) {
        sy.ci_b.push_back(ci[k]);
        sy.perm_b.push_back(k);
      }
    }
    if (ncols) sy.rp_b.push_back((int32_t)sy.ci_b.size());
  }
  if (ncols) {
    sy.lc_ptr.assign(1, 0);
    for (int i = 0; i < ncols; ++i) {
      // virtual row mpad + 16 g + i holds workgroup g's share of U[.][i]'q; the value slot behind the last entry holds 1
      for (int g = 0; g < sy.vgrid; ++g) {
        const int32_t t = nxt[sy.lcols[i]]++;
        sy.trow[t] = (int32_t)(mpad + (int64_t)kBorderMax * g + i);
        sy.tperm[t] = (int32_t)nnz;
      }
      sy.lc_row.insert(sy.lc_row.end(), lrow[i].begin(), lrow[i].end());
      sy.lc_ent.insert(sy.lc_ent.end(), lent[i].begin(), lent[i].end());
      sy.lc_ptr.push_back((int32_t)sy.lc_row.size());
    }
  }
  return std::string();
}

size_t band_factor_bytes(const fpsq_band b) { return (size_t)b->nb * b->band_w * kDB * kDB * 8; }

// Choose the formation kernel: M is formed by columns of A (k_band_form_t) when its accumulator rows fit in LDS; otherwise
// by row pairs (k_band_form), which needs the widest row span in LDS twice.  FPSQ_BAND_FORM = 1 / 2 overrides.  Non-zero
// (the handle is deleted): neither the kernel's window nor the factor fits the device.
int band_choose_form(fpsq_band b) {
  b->form_R = 16;
  while (b->form_R > 1 && b->form_R * b->band_w > 144) b->form_R /= 2;
  b->form_gen = b->band_w > 144 ? 1 : 2;
  if (const char* ev = std::getenv("FPSQ_BAND_FORM")) {
    const int want = std::atoi(ev);
    if (want == 1 || (want == 2 && b->band_w <= 144)) b->form_gen = want;
  }
  const size_t fbytes = band_factor_bytes(b);
  size_t free_b = 0, total_b = 0;
  hipMemGetInfo(&free_b, &total_b);
  if ((b->form_gen == 1 && (size_t)b->span * 16 > 150 * 1024) || fbytes + 3 * ((size_t)b->nb * kDB * kDB * 8) > free_b / 10 * 9) {
    char msg[256];
    snprintf(msg, sizeof msg, "fpsq_band_create: the banded direct path does not fit this Jacobian (half bandwidth %d "
             "blocks > 143 and a row span of %d columns > 9600, or factor storage %.1f GB of %.1f GB "
             "free): use the iterative back-end", b->band_w - 1, b->span, fbytes / 1e9, free_b / 1e9);
    g_band_create_error = msg;
    delete b;
    return FPSQ_ERR_STATE;
  }
  return FPSQ_OK;
}

// Allocate the band and the workspaces: the two streams and their events, the shared part, the structure, M, the vectors
// of a solve.  Non-zero (the handle is destroyed): failed.
int band_alloc(fpsq_band b) {
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
    g_band_create_error = "fpsq_band_create: cannot create a stream";
    delete b;
    return FPSQ_ERR_HIP;
  }
  hipStreamCreateWithFlags(&b->stream2, hipStreamNonBlocking);
  hipEventCreateWithFlags(&b->evA, hipEventDisableTiming);
  hipEventCreateWithFlags(&b->evB, hipEventDisableTiming);
  const size_t n = (size_t)b->n, m = (size_t)b->m, nz = (size_t)std::max<int64_t>(b->nnz, 1);
  const size_t tz = (size_t)std::max<int64_t>(b->t_nnz, 1);  // (= nz without long columns)
  int rc = core_setup(b, b->n);
  rc |= dalloc(b, &b->rowptr, m + 1) | dalloc(b, &b->colind, nz) | dalloc(b, &b->vals, nz + (b->cols ? 1 : 0));
  rc |= dalloc(b, &b->t_rowptr, n + 1) | dalloc(b, &b->t_colind, tz) | dalloc(b, &b->t_vals, tz);
  rc |= dalloc(b, &b->t_perm, tz) | dalloc(b, &b->rowspan, m);
  rc |= dalloc(b, &b->Mb, (size_t)b->nb * b->band_w * kDB * kDB);
  rc |= dalloc(b, &b->xn, n * 2) | dalloc(b, &b->atq, n * 2) | dalloc(b, &b->ym, (size_t)b->mpad * 2);
  if (b->reordered)
    rc |= dalloc(b, &b->rperm, m) | dalloc(b, &b->vperm, nz) | dalloc(b, &b->vals_in, nz) | dalloc(b, &b->in_bp, (size_t)b->mpad);
  if (rc) {
    g_band_create_error = b->err;
    fpsq_band_destroy(b);
    return FPSQ_ERR_HIP;
  }
  return FPSQ_OK;
}

// Upload the structure and its transpose (and the permutations of a reordered one)
void band_upload(fpsq_band b, const BandSymbolic& sy) {
  const size_t n = (size_t)b->n, m = (size_t)b->m, nnz = (size_t)b->nnz;
  if (b->reordered) {
    hipMemcpy(b->rperm, sy.rperm.data(), m * 4, hipMemcpyHostToDevice);
    if (nnz > 0) hipMemcpy(b->vperm, sy.vperm.data(), nnz * 4, hipMemcpyHostToDevice);
  }
  hipMemcpy(b->rowptr, sy.rp.data(), (m + 1) * 4, hipMemcpyHostToDevice);
  hipMemcpy(b->t_rowptr, sy.tptr.data(), (n + 1) * 4, hipMemcpyHostToDevice);
  hipMemcpy(b->rowspan, sy.span.data(), m * sizeof(int2), hipMemcpyHostToDevice);
  const size_t tnz = (size_t)b->t_nnz;
  if (nnz > 0) hipMemcpy(b->colind, sy.ci.data(), nnz * 4, hipMemcpyHostToDevice);
  if (tnz > 0) {
    hipMemcpy(b->t_colind, sy.trow.data(), tnz * 4, hipMemcpyHostToDevice);
    hipMemcpy(b->t_perm, sy.tperm.data(), tnz * 4, hipMemcpyHostToDevice);
  }
  if (b->cols) {  // the value the virtual entries of the transposed structure gather
    const double one = 1.0;
    hipMemcpy(b->vals + nnz, &one, 8, hipMemcpyHostToDevice);
  }
  hipDeviceSynchronize();
}

// The buffers of a handle with long columns: the block sweeps' own (Z = B^-1 U is one tile of them), U, Z, the factor of S, the
// partial sums, the operand with virtual rows, the columns' entries, and for k_band_form the CSR of the other columns.
// Non-zero (the handle is destroyed): failed.
int cols_setup(fpsq_band b, const BandSymbolic& sy) {
  if (b->cols == 0) return FPSQ_OK;
  b->bc_grid = sy.vgrid;
  if (!b->evS0) {  // (an arrow handle: border_setup has made them)
    hipEventCreate(&b->evS0);
    hipEventCreate(&b->evS1);
  }
  const size_t tile = (size_t)b->mpad * kBlkCols, nl = std::max<size_t>(sy.lc_row.size(), 1);
  // (an arrow handle keeps the rows' partials of the fused reduction behind the columns')
  const size_t parts = (size_t)b->bc_grid * 256 + (b->border ? (size_t)b->bd_grid * 256 : 0);
  int rc = chain16_setup(b) || dalloc(b, &b->bc_c, tile) || dalloc(b, &b->bc_z, tile) ||
           dalloc(b, &b->bc_l, (size_t)kBorderMax * kBorderMax) || dalloc(b, &b->bc_part, parts) ||
           dalloc(b, &b->bc_t, 256 + 8) || dalloc(b, &b->bd_keep, (size_t)(b->mpad + b->vrows)) ||
           dalloc(b, &b->lc_ptr, (size_t)b->cols + 1) || dalloc(b, &b->lc_row, nl) || dalloc(b, &b->lc_ent, nl) ||
           dalloc(b, &b->lc_cols, (size_t)kBorderMax);
  if (!rc && b->border) rc = dalloc(b, &b->bc_g, (size_t)kBorderMax * kBorderMax);
  if (!rc && b->form_gen == 1) {
    b->fb_nnz = (int64_t)sy.perm_b.size();
    const size_t fz = (size_t)std::max<int64_t>(b->fb_nnz, 1);
    rc = dalloc(b, &b->fb_rowptr, (size_t)b->m + 1) || dalloc(b, &b->fb_colind, fz) || dalloc(b, &b->fb_perm, fz) ||
         dalloc(b, &b->fb_vals, fz);
  }
  if (rc) {
    g_band_create_error = b->err;
    fpsq_band_destroy(b);
    return FPSQ_ERR_HIP;
  }
  hipMemset(b->bd_keep, 0, (size_t)(b->mpad + b->vrows) * 8);
  hipMemcpy(b->lc_ptr, sy.lc_ptr.data(), ((size_t)b->cols + 1) * 4, hipMemcpyHostToDevice);
  hipMemcpy(b->lc_cols, sy.lcols.data(), (size_t)b->cols * 4, hipMemcpyHostToDevice);
  if (!sy.lc_row.empty()) {
    hipMemcpy(b->lc_row, sy.lc_row.data(), sy.lc_row.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(b->lc_ent, sy.lc_ent.data(), sy.lc_ent.size() * 4, hipMemcpyHostToDevice);
  }
  if (b->form_gen == 1) {
    hipMemcpy(b->fb_rowptr, sy.rp_b.data(), ((size_t)b->m + 1) * 4, hipMemcpyHostToDevice);
    if (b->fb_nnz > 0) {
      hipMemcpy(b->fb_colind, sy.ci_b.data(), (size_t)b->fb_nnz * 4, hipMemcpyHostToDevice);
      hipMemcpy(b->fb_perm, sy.perm_b.data(), (size_t)b->fb_nnz * 4, hipMemcpyHostToDevice);
    }
  }
  hipDeviceSynchronize();
  return FPSQ_OK;
}

// The long columns' share of a factorisation, behind the band's Cholesky on b->stream: U scattered from the current values,
// Z = B^-1 U by the 16-column sweeps, the partials of U'Z, S = I + U'Z and its Cholesky.  On an arrow handle it runs behind
// border_factor: U covers the border rows too, Z_c = M_r^-1 U takes the rows' correction behind the sweeps, and G is formed
void cols_factor(fpsq_band b) {
  hipStream_t s = b->stream;
  const size_t tile = (size_t)b->mpad * kBlkCols * 8;
  if (!b->border) hipEventRecord(b->evS0, s);  // (an arrow handle: border_factor, which runs first, has recorded it)
  hipMemsetAsync(b->bc_c, 0, tile, s);
  hipLaunchKernelGGL(k_cols_scatter, dim3(b->cols, 64), dim3(256), 0, s, b->lc_ptr, b->lc_row, b->lc_ent, b->vals, b->bc_c);
  if (b->border) {  // G = U_s' - U_b'Z_r for the fused correction
    hipLaunchKernelGGL(k_border_reduce<kBlkCols>, dim3(b->bc_grid), dim3(256), 0, s, b->bc_c, b->bd_z, (int)b->mb, 0, b->bc_part,
                       b->bc_t);
    hipLaunchKernelGGL(k_arrow_g, dim3(1), dim3(256), 0, s, b->bc_part, b->bc_grid, b->bc_c, (int)b->mb, b->border, b->cols,
                       b->bc_g);
  }
  hipMemcpyAsync(b->r16, b->bc_c, tile, hipMemcpyDeviceToDevice, s);
  chain_sweeps16(b, b->Mb, b->band_w, b->chain_safe, b->chain_bw);
  if (b->border) border_correct<kBlkCols>(b, b->r16);  // (Z_c = M_r^-1 U: the rows' correction behind the sweeps)
  hipMemcpyAsync(b->bc_z, b->r16, tile, hipMemcpyDeviceToDevice, s);
  hipLaunchKernelGGL(k_border_reduce<kBlkCols>, dim3(b->bc_grid), dim3(256), 0, s, b->bc_c, b->bc_z, (int)b->m, 0, b->bc_part,
                     b->bc_t);
  hipLaunchKernelGGL(k_cols_chol, dim3(1), dim3(256), 0, s, b->bc_part, b->bc_grid, b->cols, (int)b->m, b->piv_tol, b->piv_reg,
                     b->bc_l, b->bc_t + 256, b->info_dev);
  hipEventRecord(b->evS1, s);
}

// The buffers of a bordered handle: the block sweeps' own (Z = B^-1 C is one tile of them) with the tile A multiplies, C, Z,
// the factor of S, the partial sums and the saved right-hand side of a correction.  Non-zero (the handle is destroyed): failed.
int border_setup(fpsq_band b) {
  if (b->border == 0) return FPSQ_OK;
  b->bd_grid = (int)std::max<int64_t>(1, std::min<int64_t>((b->mb + 255) / 256, kBorderGrid));
  hipEventCreate(&b->evS0);
  hipEventCreate(&b->evS1);
  const size_t tile = (size_t)b->mpad * kBlkCols;
  if (chain16_setup(b) || dalloc(b, &b->blk_xg, (size_t)b->n * kBlkCols) || dalloc(b, &b->bd_c, tile) ||
      dalloc(b, &b->bd_z, tile) || dalloc(b, &b->bd_l, (size_t)kBorderMax * kBorderMax) ||
      dalloc(b, &b->bd_part, (size_t)b->bd_grid * 256) || dalloc(b, &b->bd_t, 256)) {
    g_band_create_error = b->err;
    fpsq_band_destroy(b);
    return FPSQ_ERR_HIP;
  }
  return FPSQ_OK;
}

// The border's share of a factorisation, behind the band's Cholesky on b->stream: [C; D] = A A_s' by the block A product on
// the scattered border rows, Z = B^-1 C by the 16-column sweeps, S = D + delta I - C'Z and its Cholesky
void border_factor(fpsq_band b, double delta) {
  hipStream_t s = b->stream;
  const int mb = (int)b->mb;
  const size_t tile = (size_t)b->mpad * kBlkCols * 8;
  hipEventRecord(b->evS0, s);
  hipMemsetAsync(b->blk_xg, 0, (size_t)b->n * kBlkCols * 8, s);
  hipLaunchKernelGGL(k_border_scatter, dim3(b->border), dim3(256), 0, s, b->rowptr, b->colind, b->vals, mb, b->blk_xg);
  if (b->cols)  // (arrow: [C; D - delta I] = A_o A_s,o', the long columns belong to U)
    hipLaunchKernelGGL(k_arrow_clear, dim3(1), dim3(256), 0, s, b->lc_cols, b->cols, b->blk_xg);
  const int lgA = lane_group(b->nnz, b->m);
  WITH_LANE_GROUP(lgA, hipLaunchKernelGGL(k_bqb_prologue<LG>, dim3((unsigned)std::min<int64_t>(
                                              (b->mpad + 256 / lgA - 1) / (256 / lgA), 2048)), dim3(256), 0, s, b->rowptr,
                                          b->colind, b->vals, b->blk_xg, b->r16, (double*)nullptr, (int)b->m, (int)b->mpad))
  hipMemcpyAsync(b->bd_c, b->r16, tile, hipMemcpyDeviceToDevice, s);
  chain_sweeps16(b, b->Mb, b->band_w, b->chain_safe, b->chain_bw);
  hipMemcpyAsync(b->bd_z, b->r16, tile, hipMemcpyDeviceToDevice, s);
  hipLaunchKernelGGL(k_border_reduce<kBlkCols>, dim3(b->bd_grid), dim3(256), 0, s, b->bd_c, b->bd_z, mb, b->border, b->bd_part,
                     b->bd_t);
  hipLaunchKernelGGL(k_border_chol, dim3(1), dim3(256), 0, s, b->bd_part, b->bd_grid, b->bd_c, mb, b->border, delta, b->piv_tol,
                     b->piv_reg, b->bd_l, b->info_dev);
  if (!b->cols) hipEventRecord(b->evS1, s);  // (an arrow handle: cols_factor, which runs next, records it)
}

// the check of max_cols every entry that takes it makes before anything else: null = fine
const char* bad_max_cols(int32_t max_border, int32_t max_cols, bool arrow) {
  if (max_cols < 0 || max_cols > kBorderMax) return "max_cols must be 0 .. 16";
  if (!arrow && max_border > 0 && max_cols > 0)
    return "max_border > 0 together with max_cols > 0: a handle takes one kind of border, rows or columns";
  return nullptr;
}

int band_analyze(int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t max_border, int32_t max_cols,
                 bool arrow, int32_t* row_perm, int32_t* long_cols, fpsq_band_info* info);
int band_create(fpsq_band* out, int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t max_border,
                int32_t max_cols, bool arrow, int32_t device);
int band_create_coo(fpsq_band* out, int64_t n, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                    int32_t index_base, int32_t max_border, int32_t max_cols, bool arrow, int32_t device);
int band_factor_numeric(fpsq_band b, double delta, int32_t* info);
}  // namespace

extern "C" {

const char* fpsq_band_last_error(fpsq_band b) { return b ? b->err.c_str() : g_band_create_error.c_str(); }

int fpsq_band_analyze(int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t* row_perm,
                      fpsq_band_info* info) {
  return fpsq_band_analyze_bordered(n, m, rowptr, colind, 0, row_perm, info);
}

int fpsq_band_analyze_bordered(int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t max_border,
                               int32_t* row_perm, fpsq_band_info* info) {
  return fpsq_band_analyze_bordered_cols(n, m, rowptr, colind, max_border, 0, row_perm, nullptr, info);
}

int fpsq_band_analyze_bordered_cols(int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t max_border,
                                    int32_t max_cols, int32_t* row_perm, int32_t* long_cols, fpsq_band_info* info) {
  return band_analyze(n, m, rowptr, colind, max_border, max_cols, false, row_perm, long_cols, info);
}

int fpsq_band_analyze_arrow(int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t max_border,
                            int32_t max_cols, int32_t* row_perm, int32_t* long_cols, fpsq_band_info* info) {
  return band_analyze(n, m, rowptr, colind, max_border, max_cols, true, row_perm, long_cols, info);
}
}  // extern "C"

namespace {
int band_analyze(int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t max_border, int32_t max_cols,
                 bool arrow, int32_t* row_perm, int32_t* long_cols, fpsq_band_info* info) {
  if (max_border < 0 || max_border > kBorderMax) {
    g_band_create_error = "fpsq_band_analyze: max_border must be 0 .. 16";
    return FPSQ_ERR_ARG;
  }
  if (const char* what = bad_max_cols(max_border, max_cols, arrow)) {
    g_band_create_error = std::string("fpsq_band_analyze: ") + what;
    return FPSQ_ERR_ARG;
  }
  if (n <= 0 || m <= 0 || !rowptr || n >= INT32_MAX || m >= INT32_MAX - 256 || rowptr[0] != 0) {
    g_band_create_error = "fpsq_band_analyze: bad arguments (0-based CSR in HOST memory expected)";
    return FPSQ_ERR_ARG;
  }
  std::vector<int32_t> rp(rowptr, rowptr + m + 1);
  for (int64_t i = 0; i < m; ++i)
    if (rp[i + 1] < rp[i]) {
      g_band_create_error = "fpsq_band_analyze: rowptr not monotone";
      return FPSQ_ERR_ARG;
    }
  const int64_t nnz = rp[m];
  if (nnz > 0 && !colind) {
    g_band_create_error = "fpsq_band_analyze: colind missing";
    return FPSQ_ERR_ARG;
  }
  std::vector<int32_t> ci(colind, colind + nnz), rperm_h, vperm_h;
  ci.resize(std::max<int64_t>(nnz, 1));
  int chain_safe = 0, chain_bw = 0, border = 0;
  std::vector<int32_t> lcols;
  const std::string msg =
      arrow ? band_order_arrow(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw, max_border, max_cols, border, lcols)
      : max_cols > 0 ? band_order_cols(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw, max_cols, lcols)
                     : band_order(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw, max_border, border);
  if (!msg.empty()) {
    g_band_create_error = msg;
    return FPSQ_ERR_ARG;
  }
  if (long_cols)
    for (int i = 0; i < kBorderMax; ++i) long_cols[i] = i < (int)lcols.size() ? lcols[i] : -1;
  if (!lcols.empty()) {  // the band is that of the other columns: drop the long ones from the structure that is measured
    std::vector<char> out(n, 0);
    for (int32_t c : lcols) out[c] = 1;
    int32_t w = 0;
    for (int64_t i = 0, k = 0; i < m; ++i) {
      for (const int32_t e = rp[i + 1]; k < e; ++k)
        if (!out[ci[k]]) ci[w++] = ci[k];
      rp[i + 1] = w;
    }
  }
  if (row_perm)
    for (int64_t p = 0; p < m; ++p) row_perm[p] = rperm_h.empty() ? (int32_t)p : rperm_h[p];
  if (info) {
    const int64_t mb = m - border;
    const int64_t nb = (mb + kDB - 1) / kDB;
    const int64_t bwb = std::min(band_blocks(n, mb, rp, ci), nb - 1);
    *info = fpsq_band_info{};
    info->n = n;
    info->m = m;
    info->nnz = nnz;
    info->border_cols = (int64_t)lcols.size();
    info->border_pivot_ratio = 1.0;
    info->nblocks = nb;
    info->bandwidth_blocks = bwb;
    info->factor_bytes = nb * (bwb + 1) * (int64_t)kDB * kDB * 8;
    info->reordered = rperm_h.empty() ? 0 : 1;
    info->chains = chain_safe > 0 ? 2 : 1;
    info->border_rows = border;
  }
  return FPSQ_OK;
}
}  // namespace

extern "C" {

int fpsq_band_destroy(fpsq_band b) {
  if (!b) return FPSQ_ERR_ARG;
  core_teardown(b);
  if (b->evA) hipEventDestroy(b->evA);
  if (b->evB) hipEventDestroy(b->evB);
  if (b->evS0) hipEventDestroy(b->evS0);
  if (b->evS1) hipEventDestroy(b->evS1);
  if (b->og_scal_host) hipHostFree(b->og_scal_host);
  if (b->stream2) {
    hipStreamSynchronize(b->stream2);
    hipStreamDestroy(b->stream2);
  }
  delete b;
  return FPSQ_OK;
}

int fpsq_band_create(fpsq_band* out, int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t device) {
  return fpsq_band_create_bordered(out, n, m, rowptr, colind, 0, device);
}

int fpsq_band_create_bordered(fpsq_band* out, int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind,
                              int32_t max_border, int32_t device) {
  return fpsq_band_create_bordered_cols(out, n, m, rowptr, colind, max_border, 0, device);
}

int fpsq_band_create_bordered_cols(fpsq_band* out, int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind,
                                   int32_t max_border, int32_t max_cols, int32_t device) {
  return band_create(out, n, m, rowptr, colind, max_border, max_cols, false, device);
}

int fpsq_band_create_arrow(fpsq_band* out, int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind,
                           int32_t max_border, int32_t max_cols, int32_t device) {
  return band_create(out, n, m, rowptr, colind, max_border, max_cols, true, device);
}
}  // extern "C"

namespace {
int band_create(fpsq_band* out, int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t max_border,
                int32_t max_cols, bool arrow, int32_t device) {
  if (max_border < 0 || max_border > kBorderMax) {
    g_band_create_error = "fpsq_band_create: max_border must be 0 .. 16";
    return FPSQ_ERR_ARG;
  }
  if (const char* what = bad_max_cols(max_border, max_cols, arrow)) {
    g_band_create_error = std::string("fpsq_band_create: ") + what;
    return FPSQ_ERR_ARG;
  }
  if (!out || n <= 0 || m <= 0 || !rowptr || n >= INT32_MAX || m >= INT32_MAX - 256) {
    g_band_create_error = "fpsq_band_create: bad arguments";
    return FPSQ_ERR_ARG;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    g_band_create_error = std::string("fpsq_band_create: no HIP device (") + hipGetErrorString(e) +
                          "); libfpsq has no CPU fallback";
    return FPSQ_ERR_HIP;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_band_create_error = "fpsq_band_create: cannot select the device";
    return FPSQ_ERR_HIP;
  }
  BandSymbolic sy;
  const std::string msg = band_symbolic(n, m, rowptr, colind, max_border, max_cols, arrow, sy);
  if (!msg.empty()) {
    g_band_create_error = msg;
    return FPSQ_ERR_ARG;
  }
  fpsq_band b = new fpsq_band_s();
  b->name = "band";
  b->n = n;
  b->m = m;
  b->nnz = sy.rp[m];
  b->device = device;
  b->border = sy.border;
  b->mb = m - sy.border;
  b->cols = (int)sy.lcols.size();
  b->t_nnz = sy.t_nnz;
  b->vrows = (int64_t)kBorderMax * sy.vgrid;
  b->mpad = (m + kDB - 1) / kDB * kDB;
  b->nb = (b->mb + kDB - 1) / kDB;  // (the blocks of the band rows; = mpad / 128 without a border)
  b->band_w = (int)std::min<int64_t>(sy.bwb, b->nb - 1) + 1;
  b->span = sy.maxspan;
  b->chain_safe = sy.chain_safe;
  b->chain_bw = std::min(sy.chain_bw, (b->band_w - 1) / 2);
  b->reordered = !sy.rperm.empty();
  b->rperm_host = sy.rperm;
  if (const char* ev = std::getenv("FPSQ_ARROW_FUSED")) b->arrow_fused = std::atoi(ev) != 0;
  if (int rc = band_choose_form(b)) return rc;
  if (int rc = band_alloc(b)) return rc;
  band_upload(b, sy);
  if (int rc = border_setup(b)) {
    *out = nullptr;
    return rc;
  }
  if (int rc = cols_setup(b, sy)) {
    *out = nullptr;
    return rc;
  }
  hipFuncSetAttribute((const void*)k_potrf_inv128m, hipFuncAttributeMaxDynamicSharedMemorySize, kPotrfLds5);
  hipFuncSetAttribute((const void*)k_gemm128_lds<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kG128Lds0);
  hipFuncSetAttribute((const void*)k_gemm128_lds<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kG128Lds1);
  if (b->form_gen == 1)
    hipFuncSetAttribute((const void*)k_band_form, hipFuncAttributeMaxDynamicSharedMemorySize, b->span * 16);
  else
    hipFuncSetAttribute((const void*)k_band_form_t, hipFuncAttributeMaxDynamicSharedMemorySize,
                        b->form_R * b->band_w * kDB * 8);
  b->info.n = n;
  b->info.m = m;
  b->info.nnz = b->nnz;
  b->info.nblocks = b->nb;
  b->info.bandwidth_blocks = b->band_w - 1;
  b->info.reordered = b->reordered ? 1 : 0;
  b->info.chains = b->chain_safe > 0 ? 2 : 1;
  b->info.factor_bytes = (int64_t)band_factor_bytes(b);
  b->info.border_rows = b->border;
  b->info.border_cols = b->cols;
  b->info.border_pivot_ratio = 1.0;
  *out = b;
  return FPSQ_OK;
}
}  // namespace

extern "C" {

int fpsq_band_create_coo(fpsq_band* out, int64_t n, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                         int32_t index_base, int32_t device) {
  return fpsq_band_create_coo_bordered(out, n, m, nnz, rows, cols, index_base, 0, device);
}

int fpsq_band_create_coo_bordered(fpsq_band* out, int64_t n, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                                  int32_t index_base, int32_t max_border, int32_t device) {
  return fpsq_band_create_coo_bordered_cols(out, n, m, nnz, rows, cols, index_base, max_border, 0, device);
}

int fpsq_band_create_coo_bordered_cols(fpsq_band* out, int64_t n, int64_t m, int64_t nnz, const int64_t* rows,
                                       const int64_t* cols, int32_t index_base, int32_t max_border, int32_t max_cols,
                                       int32_t device) {
  return band_create_coo(out, n, m, nnz, rows, cols, index_base, max_border, max_cols, false, device);
}

int fpsq_band_create_coo_arrow(fpsq_band* out, int64_t n, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                               int32_t index_base, int32_t max_border, int32_t max_cols, int32_t device) {
  return band_create_coo(out, n, m, nnz, rows, cols, index_base, max_border, max_cols, true, device);
}
}  // extern "C"

namespace {
int band_create_coo(fpsq_band* out, int64_t n, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                    int32_t index_base, int32_t max_border, int32_t max_cols, bool arrow, int32_t device) {
  if (max_border < 0 || max_border > kBorderMax) {
    g_band_create_error = "fpsq_band_create_coo: max_border must be 0 .. 16";
    return FPSQ_ERR_ARG;
  }
  if (const char* what = bad_max_cols(max_border, max_cols, arrow)) {
    g_band_create_error = std::string("fpsq_band_create_coo: ") + what;
    return FPSQ_ERR_ARG;
  }
  if (!out || n <= 0 || m <= 0 || nnz < 0 || nnz >= INT32_MAX || (nnz > 0 && (!rows || !cols))) {
    g_band_create_error = "fpsq_band_create_coo: bad arguments";
    return FPSQ_ERR_ARG;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_band_create_error = "fpsq_band_create_coo: cannot select the device";
    return FPSQ_ERR_HIP;
  }
  std::vector<int64_t> r(nnz), c(nnz);
  if (nnz && (hipMemcpy(r.data(), rows, (size_t)nnz * 8, hipMemcpyDefault) != hipSuccess ||
              hipMemcpy(c.data(), cols, (size_t)nnz * 8, hipMemcpyDefault) != hipSuccess)) {
    g_band_create_error = "fpsq_band_create_coo: cannot read the triplets";
    return FPSQ_ERR_ARG;
  }
  std::vector<int32_t> order, slotptr, srow, scol;
  const std::string msg = coo_sort(m, n, nnz, r.data(), c.data(), index_base, order, slotptr, srow, scol);
  if (!msg.empty()) {
    g_band_create_error = "fpsq_band_create_coo: " + msg;
    return FPSQ_ERR_ARG;
  }
  const int64_t ns = (int64_t)srow.size();
  std::vector<int32_t> rp(m + 1, 0);
  for (int64_t i = 0; i < ns; ++i) rp[srow[i] + 1]++;
  for (int64_t i = 0; i < m; ++i) rp[i + 1] += rp[i];
  if (int rc = band_create(out, n, m, rp.data(), scol.data(), max_border, max_cols, arrow, device)) return rc;
  fpsq_band b = *out;
  const bool dup = ns != nnz;
  if (dalloc(b, &b->coo_perm, (size_t)std::max<int64_t>(nnz, 1)) || dalloc(b, &b->coo_in, (size_t)std::max<int64_t>(nnz, 1)) ||
      dalloc(b, &b->csr_in, (size_t)std::max<int64_t>(ns, 1)) || (dup && dalloc(b, &b->coo_slotptr, slotptr.size()))) {
    g_band_create_error = b->err;
    fpsq_band_destroy(b);
    *out = nullptr;
    return FPSQ_ERR_HIP;
  }
  if (nnz) hipMemcpy(b->coo_perm, order.data(), (size_t)nnz * 4, hipMemcpyHostToDevice);
  if (dup) hipMemcpy(b->coo_slotptr, slotptr.data(), slotptr.size() * 4, hipMemcpyHostToDevice);
  hipDeviceSynchronize();
  b->coo_nnz = nnz;
  return FPSQ_OK;
}
}  // namespace

extern "C" {

int fpsq_band_factorize_coo(fpsq_band b, const double* vals, double delta, int32_t* info) {
  if (!b || b->coo_nnz < 0 || (!vals && b->coo_nnz > 0)) {
    if (b) b->err = "band_factorize_coo: the handle was not created with fpsq_band_create_coo, or null values";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(b->device);
  if (int rc = wait_input(b)) return rc;
  if (b->coo_nnz > 0)
    if (int rc = coo_to_slots(b, vals, nullptr, b->csr_in, b->nnz)) return rc;
  return fpsq_band_factorize(b, b->csr_in, delta, info);  // (same stream: the slots are complete when it reads them)
}

int fpsq_band_set_regularization(fpsq_band b, double tol, double reg) { return set_regularization(b, tol, reg); }

int fpsq_band_factorize(fpsq_band b, const double* vals, double delta, int32_t* info) {
  if (!b || (!vals && b->nnz > 0) || !(delta >= 0.0)) return FPSQ_ERR_ARG;
  hipSetDevice(b->device);
  hipStream_t s = b->stream;
  b->factored = false;
  if (int rc = wait_input(b)) return rc;  // (device-resident values produced on a stream registered with fpsq_band_set_input_stream)
  b->have_vals = true;
  if (b->nnz > 0) {
    if (b->reordered) {
      CHK(b, hipMemcpyAsync(b->vals_in, vals, (size_t)b->nnz * 8, hipMemcpyDefault, s));
      hipLaunchKernelGGL(k_gather_d, dim3((unsigned)std::min<int64_t>((b->nnz + 255) / 256, 4096)), dim3(256), 0, s, b->vals_in,
                         b->vperm, b->vals, b->nnz);
    } else {
      CHK(b, hipMemcpyAsync(b->vals, vals, (size_t)b->nnz * 8, hipMemcpyDefault, s));
    }
    hipLaunchKernelGGL(k_gather_d, dim3((unsigned)std::min<int64_t>((b->t_nnz + 255) / 256, 4096)), dim3(256), 0, s, b->vals,
                       b->t_perm, b->t_vals, b->t_nnz);
    if (b->fb_nnz > 0)  // (long columns and k_band_form: the values of the other columns alone)
      hipLaunchKernelGGL(k_gather_d, dim3((unsigned)std::min<int64_t>((b->fb_nnz + 255) / 256, 4096)), dim3(256), 0, s, b->vals,
                         b->fb_perm, b->fb_vals, b->fb_nnz);
  }
  return band_factor_numeric(b, delta, info);
}
}  // extern "C"

namespace {
// The numeric phase of a factorisation on the values that lie in vals / t_vals [/ fb_vals] (fpsq_band_factorize uploads them,
// fpsq_band_nlp_objgrad writes them in place): form, Cholesky, factor_end.  Synchronous; the return value and *info are
// fpsq_band_factorize's.
int band_factor_numeric(fpsq_band b, double delta, int32_t* info) {
  hipStream_t s = b->stream;
  const int nb = (int)b->nb, W = b->band_w, bw = W - 1;
  ++b->fact_gen;
  CHK(b, hipMemsetAsync(b->info_dev, 0, 8, s));
  CHK(b, hipMemsetAsync(b->Mb, 0, (size_t)nb * W * kDB * kDB * 8, s));
  hipEventRecord(b->e0, s);
  // numeric phase 1: M = A A' + delta I into the band (jac_coord! + sparse(...) of src/solve_linear_system.jl:223-233)
  // (with long columns both kernels form B: k_band_form on the CSR of the other columns, k_band_form_t by its j <= i guard)
  if (b->form_gen == 1)
    hipLaunchKernelGGL(k_band_form, dim3(nb), dim3(256), (size_t)b->span * 16, s, b->cols ? b->fb_rowptr : b->rowptr,
                       b->cols ? b->fb_colind : b->colind, b->cols ? b->fb_vals : b->vals, b->rowspan, (int)b->mb, nb * kDB, W,
                       delta, b->Mb, b->span);
  else
    hipLaunchKernelGGL(k_band_form_t, dim3(nb), dim3(256), (size_t)b->form_R * W * kDB * 8, s, b->rowptr, b->colind, b->vals,
                       b->t_rowptr, b->t_colind, b->t_vals, (int)b->mb, nb * kDB, W, delta, b->Mb, b->form_R);
  hipEventRecord(b->e1, s);
  // numeric phase 2: right-looking block-banded Cholesky (ldl_factorize!, :234), the dense back-end's block kernels.
  // One step: diagonal block k, panel blocks (k + st j, k) and trailing blocks (k + st i, k + st j), 1 <= j <= i <= rem
  // (st = 1: the whole band below k; st = 2: the blocks of k's own chain)
  auto step = [&](hipStream_t q, int k, int st, int rem) {
    double* inv = launch_potrf(b, q, b->Mb + blk_off(b, k, k), kDB, k);
    if (rem <= 0) return;
    BlockStrides ps, ts;
    ps.on = ts.on = 1;
    ps.a = ps.ci = (size_t)st * bw * kDB * kDB;  // block (k + st (1 + bi), k): st block rows down, st columns of the band left
    ps.b = ps.cj = 0;
    ts.a = ts.b = ts.ci = ps.a;
    ts.cj = (size_t)st * kDB * kDB;
    double* panel = b->Mb + blk_off(b, k + st, k);
    double* trail = b->Mb + blk_off(b, k + st, k + st);
    hipLaunchKernelGGL(k_gemm128_lds<1>, dim3(1, 4 * rem), dim3(1024), kG128Lds1, q, panel, kDB, panel, kDB, inv, kDB, ps);
    hipLaunchKernelGGL(k_gemm128_lds<0>, dim3(2 * rem, 2 * rem), dim3(1024), kG128Lds0, q, trail, kDB, panel, kDB, panel, kDB, ts);
  };
  int k0 = 0;
  if (b->chain_safe > 0) {  // the two chains side by side
    hipStream_t s2 = b->stream2;
    hipEventRecord(b->evA, s);
    hipStreamWaitEvent(s2, b->evA, 0);
    for (int c = 0; c < b->chain_safe; ++c) {
      step(s, 2 * c, 2, b->chain_bw);
      step(s2, 2 * c + 1, 2, b->chain_bw);
    }
    hipEventRecord(b->evB, s2);
    hipStreamWaitEvent(s, b->evB, 0);
    k0 = 2 * b->chain_safe;
  }
  for (int k = k0; k < nb; ++k) step(s, k, 1, std::min(bw, nb - 1 - k));
  if (b->border) border_factor(b, delta);
  if (b->cols) cols_factor(b);
  int32_t pivot = 0;
  const int rc = factor_end(b, &b->info.last_form_ms, &b->info.last_chol_ms, &b->info.regularized_pivots, &pivot);
  if (b->border || b->cols) {
    // the sweeps that formed Z may have raised the error word: it is looked at and cleared HERE, whatever the code above, so
    // that it never surfaces as the time-out of a later, unrelated solve
    const bool expired = *b->chain_err != 0;
    *b->chain_err = 0;
    if (rc >= 0) {
      float ms = 0.f;
      hipEventElapsedTime(&ms, b->evS0, b->evS1);
      b->info.last_border_ms = ms;
      b->info.last_chol_ms -= ms;  // (the band's Cholesky alone, as on a handle without a border)
      if (b->cols) CHK(b, hipMemcpy(&b->info.border_pivot_ratio, b->bc_t + 256, 8, hipMemcpyDeviceToHost));
      if (expired) {
        b->factored = false;
        b->err = "band_factorize: Z = B^-1 C did not arrive (bounded wait of the block sweep expired)";
        return FPSQ_ERR_TIMEOUT;
      }
    }
  }
  if (rc >= 0 && info)  // (first non-positive pivot, 1-based, in the CALLER's row numbering)
    *info = pivot > 0 && b->reordered && pivot <= (int32_t)b->m ? b->rperm_host[pivot - 1] + 1 : pivot;
  return rc;
}
}  // namespace

extern "C" {

int fpsq_band_solve_two_mixed(fpsq_band b, const double* rhs1, const double* rhs2, double* p1, double* q1, double* p2,
                              double* q2) {
  if (int rc = solve_begin(b, true, rhs1, rhs2, p1, q1, p2, q2)) return rc;
  hipStream_t s = b->stream;
  // r = [A g, -c]:  q1 = M^-1 A g,  q2 = -M^-1 c;  then p1 = g - A'q1, p2 = -A'q2   
  hipLaunchKernelGGL(k_dense_pack2, grid256(b->n), dim3(256), 0, s, b->in_a, 1.0,
                     (const double*)nullptr, 0.0, b->xn, (int)b->n, (int)b->n);
  hipLaunchKernelGGL(k_csr_mv2, grid256(b->m), dim3(256), 0, s, b->rowptr, b->colind, b->vals, b->xn,
                     b->ym, (int)b->m);
  const double* cperm = b->in_b;
  if (b->reordered) {
    hipLaunchKernelGGL(k_gather_d, grid256(b->m), dim3(256), 0, s, b->in_b, b->rperm, b->in_bp, b->m);
    cperm = b->in_bp;
  }
  hipLaunchKernelGGL(k_band_rhs, grid256(b->mpad), dim3(256), 0, s, b->ym, 0, cperm, -1.0, b->r2,
                     (int)b->m, (int)b->mpad, 0);
  return band_finish(b, nullptr, p1, q1, p2, q2);
}

int fpsq_band_solve_two_least_squares(fpsq_band b, const double* rhs1, const double* rhs2, double* p1, double* q1,
                                      double* p2, double* q2) {
  if (int rc = solve_begin(b, false, rhs1, rhs2, p1, q1, p2, q2)) return rc;
  hipStream_t s = b->stream;
  hipLaunchKernelGGL(k_dense_pack2, grid256(b->n), dim3(256), 0, s, b->in_a, 1.0, b->in_b, 1.0, b->xn,
                     (int)b->n, (int)b->n);
  hipLaunchKernelGGL(k_csr_mv2, grid256(b->m), dim3(256), 0, s, b->rowptr, b->colind, b->vals, b->xn,
                     b->ym, (int)b->m);
  hipLaunchKernelGGL(k_band_rhs, grid256(b->mpad), dim3(256), 0, s, b->ym, 0, (const double*)nullptr,
                     0.0, b->r2, (int)b->m, (int)b->mpad, 1);
  return band_finish(b, b->in_b, p1, q1, p2, q2);
}

int fpsq_band_get_info(fpsq_band b, fpsq_band_info* info) {
  if (!b || !info) return FPSQ_ERR_ARG;
  *info = b->info;
  return FPSQ_OK;
}
}  // extern "C"


// ------------------------------------------------------------- device-resident eq-QP evaluations on the banded handle

namespace {
constexpr int kBqMaxGrid = 2048;  // workgroups of a product kernel: 256 CUs x 8 resident workgroups of 256 threads

int bq_grid(int64_t rows, int lg) { return (int)std::min<int64_t>((rows + 256 / lg - 1) / (256 / lg), kBqMaxGrid); }

// The launches between the arguments and the outputs of an evaluation, left in flight on b->stream: [pack,] the A product
// that writes the right-hand sides of the M-solves where the sweeps read them, the sweeps, the A' product with the row
// epilogue.  hp: hprod (x = v, out = Hv), else objgrad (out = grad phi).  All pointers are device pointers.
void bq_launches(fpsq_band b, fpsq_band_qp qp, bool hp, const double* x, const double* xk, double sigma, double rho,
                 double eta, double* out, double* gs, double* ys) {
  hipStream_t s = b->stream;
  const int n = (int)b->n, m = (int)b->m, mpad = (int)b->mpad;
  double* keep = b->cols ? b->bd_keep : b->o_q2;  // (long columns: the operand has virtual rows)
  if (qp->sparse_q) {
    WITH_LANE_GROUP(qp->lgR, WITH_BOOL(hp, HP, hipLaunchKernelGGL((k_bq_pack_sq<LG, HP>), dim3(qp->gridR), dim3(256), 0, s,
                                                                  qp->r_rowptr, qp->r_colind, qp->r_vals, x, qp->q, qp->d,
                                                                  b->xn, qp->partF, n)))
    if (hp && qp->long_rows)  // (R v)_T of the long rows, before the A product reads xn
      hipLaunchKernelGGL(k_bq_long_rows<LR_PACK>, dim3(qp->long_rows->cols), dim3(256), 0, s, *qp->long_rows, x,
                         (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, 0.0, b->xn);
  } else if (!qp->gather_g) {
    WITH_BOOL(hp, HP, hipLaunchKernelGGL(k_bq_pack<HP>, grid256(n), dim3(256), 0, s, x, qp->q, qp->d, b->xn, n))
  }
  WITH_LANE_GROUP(qp->lgA, WITH_BOOL(hp, HP, WITH_BOOL(qp->gather_g, GM, hipLaunchKernelGGL(
      (k_bq_prologue<LG, HP, GM>), dim3(qp->gridP), dim3(256), 0, s, b->rowptr, b->colind, b->vals, b->xn, x, qp->q, qp->d,
      qp->bp, b->r2, keep, qp->partP, m, mpad, n))))
  if (b->cols) cols_keep<1>(b, keep);
  band_solve(b);
  if (!qp->sparse_q) {
    WITH_LANE_GROUP(qp->lgT, WITH_BOOL(hp, HP, hipLaunchKernelGGL(
        (k_bq_epilogue<LG, HP>), dim3(qp->gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals, b->r2, keep,
        b->row_perm(), x, xk, qp->q, qp->d, sigma, rho, eta, out, gs, ys, qp->partE, n, m)))
    return;
  }
  WITH_LANE_GROUP(qp->lgT, WITH_BOOL(hp, HP, hipLaunchKernelGGL(
      (k_bq_epilogue_sq<LG, HP>), dim3(qp->gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals, b->r2, keep,
      b->row_perm(), xk, qp->q, b->xn, sigma, rho, eta, out, gs, ys, qp->tv, qp->partE, n, m)))
  if (out) {  // out -= R p2 (objgrad) resp. R Ptv (hprod): the rows of tv are complete only now
    WITH_LANE_GROUP(qp->lgR, hipLaunchKernelGGL(k_bq_jacmul<LG>, dim3(qp->gridR), dim3(256), 0, s, qp->r_rowptr, qp->r_colind,
                                                qp->r_vals, (const int32_t*)nullptr, (const int32_t*)nullptr, -1.0, qp->tv, 1.0,
                                                out, n))
    if (hp && qp->long_rows)
      hipLaunchKernelGGL(k_bq_long_rows<LR_HV2>, dim3(qp->long_rows->cols), dim3(256), 0, s, *qp->long_rows, x,
                         (const double*)qp->tv, (const double*)nullptr, (const double*)nullptr, rho, out);
  }
}

// Device buffers of a model, owned by its list (fpsq_band_qp_destroy frees them): all are allocated, then those with a
// source are filled from it.  False: a call failed.
struct QpBuf { void** p; size_t bytes; const void* src; hipMemcpyKind kind; };

template <class Model>
bool qp_buffers(Model* qp, std::initializer_list<QpBuf> bufs) {
  for (const QpBuf& u : bufs) {
    if (hipMalloc(u.p, u.bytes) != hipSuccess) return false;
    qp->allocs.push_back(*u.p);
  }
  for (const QpBuf& u : bufs)
    if (u.src && hipMemcpy(*u.p, u.src, u.bytes, u.kind) != hipSuccess) return false;
  return true;
}
}  // namespace

extern "C" {

int fpsq_band_set_input_stream(fpsq_band b, int32_t enabled, void* hip_stream) {
  return set_input_stream(b, enabled, hip_stream);
}

int fpsq_band_qp_create(fpsq_band b, const double* qdiag, const double* d, const double* bvec, fpsq_band_qp* out) {
  if (!b || !qdiag || !d || !bvec || !out) return FPSQ_ERR_ARG;
  hipSetDevice(b->device);
  if (!b->scal) {  // the scalars of a call: device side and pinned host side
    if (dalloc(b, &b->scal, 8)) return FPSQ_ERR_HIP;
    CHK(b, hipHostMalloc((void**)&b->scal_host, 64, hipHostMallocDefault));
  }
  std::vector<double> bh((size_t)b->m), bs((size_t)b->m);
  CHK(b, hipMemcpy(bh.data(), bvec, (size_t)b->m * 8, hipMemcpyDefault));
  for (int64_t p = 0; p < b->m; ++p) bs[p] = bh[b->reordered ? b->rperm_host[p] : p];
  fpsq_band_qp qp = new fpsq_band_qp_s();
  qp->b = b;
  qp->lgA = lane_group(b->nnz, b->m);
  qp->lgT = lane_group(b->nnz, b->n);
  qp->gridP = bq_grid(b->mpad, qp->lgA);
  qp->gridE = bq_grid(b->n, qp->lgT);
  if (const char* e = getenv("FPSQ_BAND_QP_G")) qp->gather_g = atoi(e) != 0;
  const size_t nb8 = (size_t)b->n * 8, mb8 = (size_t)b->m * 8;
  if (!qp_buffers(qp, {{(void**)&qp->q, nb8, qdiag, hipMemcpyDefault},
                       {(void**)&qp->d, nb8, d, hipMemcpyDefault},
                       {(void**)&qp->bp, mb8, bs.data(), hipMemcpyHostToDevice},
                       {(void**)&qp->partP, (size_t)qp->gridP * 16, nullptr, hipMemcpyDefault},
                       {(void**)&qp->partE, (size_t)qp->gridE * 16, nullptr, hipMemcpyDefault}})) {
    b->err = "band_qp_create: cannot allocate or fill the model's vectors";
    fpsq_band_qp_destroy(qp);
    return FPSQ_ERR_HIP;
  }
  *out = qp;
  return FPSQ_OK;
}

int fpsq_band_qp_create_csr(fpsq_band b, const int32_t* q_rowptr, const int32_t* q_colind, const double* q_vals,
                            const double* d, const double* bvec, fpsq_band_qp* out) {
  if (!b || !q_rowptr || !d || !bvec || !out) return FPSQ_ERR_ARG;
  hipSetDevice(b->device);
  const int64_t n = b->n;
  auto bad = [&](const std::string& what) {
    b->err = "band_qp_create_csr: " + what;
    return FPSQ_ERR_ARG;
  };
  // Q on the host, once: the checks (the kernels read rows only, so an unsymmetric Q would give a wrong Hessian silently)
  // and the split Q = diag(q) + R  (fpsq_qcsr.h)
  std::vector<int32_t> rp((size_t)n + 1);
  CHK(b, hipMemcpy(rp.data(), q_rowptr, ((size_t)n + 1) * 4, hipMemcpyDefault));
  if (const std::string what = qcsr_check_rowptr(n, rp.data()); !what.empty()) return bad(what);
  const size_t nnz = (size_t)rp[n];
  if (nnz && (!q_colind || !q_vals)) return FPSQ_ERR_ARG;
  std::vector<int32_t> ci(nnz);
  std::vector<double> va(nnz);
  if (nnz) {
    CHK(b, hipMemcpy(ci.data(), q_colind, nnz * 4, hipMemcpyDefault));
    CHK(b, hipMemcpy(va.data(), q_vals, nnz * 8, hipMemcpyDefault));
  }
  QcsrSplit sp;
  if (const std::string what = qcsr_check_split(n, rp.data(), ci.data(), va.data(), sp); !what.empty()) return bad(what);
  const std::vector<double>&qd = sp.qd, &rv = sp.rv;
  const std::vector<int32_t>&rrp = sp.rrp, &rci = sp.rci;
  fpsq_band_qp qp = nullptr;
  if (int rc = fpsq_band_qp_create(b, qd.data(), d, bvec, &qp)) return rc;
  const size_t rnz = rci.size();
  qp->sparse_q = true;
  qp->gather_g = false;  // (FPSQ_BAND_QP_G has no meaning here: g needs a product with R)
  qp->lgR = lane_group((int64_t)rnz, n);
  qp->gridR = bq_grid(n, qp->lgR);
  if (!qp_buffers(qp, {{(void**)&qp->r_rowptr, ((size_t)n + 1) * 4, rrp.data(), hipMemcpyHostToDevice},
                       {(void**)&qp->r_colind, std::max<size_t>(rnz, 1) * 4, rnz ? rci.data() : nullptr, hipMemcpyHostToDevice},
                       {(void**)&qp->r_vals, std::max<size_t>(rnz, 1) * 8, rnz ? rv.data() : nullptr, hipMemcpyHostToDevice},
                       {(void**)&qp->tv, (size_t)n * 8, nullptr, hipMemcpyDefault},
                       {(void**)&qp->partF, (size_t)qp->gridR * 8, nullptr, hipMemcpyDefault}})) {
    b->err = "band_qp_create_csr: cannot allocate or fill the objective Hessian";
    fpsq_band_qp_destroy(qp);
    return FPSQ_ERR_HIP;
  }
  *out = qp;
  return FPSQ_OK;
}

int fpsq_band_qp_destroy(fpsq_band_qp qp) {
  if (!qp) return FPSQ_ERR_ARG;
  for (void* p : qp->allocs) hipFree(p);
  delete qp;
  return FPSQ_OK;
}

int fpsq_band_qp_objgrad(fpsq_band b, fpsq_band_qp qp, const double* x, double sigma, double rho, double eta, const double* xk,
                         double* fx, double* gx, double* ys, double* gs) {
  if (!b || !qp || qp->b != b || !x || !fx) return FPSQ_ERR_ARG;
  if (int rc = eval_begin(b)) return rc;
  rho = rho > 0.0 ? rho : 0.0;  // (the reference adds these terms only when the parameter is positive)
  eta = eta > 0.0 ? eta : 0.0;
  const size_t n = (size_t)b->n, m = (size_t)b->m;
  const StagedArg ax = staged(b, x, b->in_a, n);
  if (int rc = stage_in(b, ax)) return rc;
  const StagedArg axk = staged(b, eta > 0.0 ? xk : nullptr, b->in_b, n);
  if (int rc = stage_in(b, axk)) return rc;
  const StagedArg ogx = staged(b, gx, b->o_p1, n), ogs = staged(b, gs, b->o_p2, n), oys = staged(b, ys, b->o_q1, m);
  bq_launches(b, qp, false, ax.tile(), axk.tile(), sigma, rho, eta, ogx.tile(), ogs.tile(), oys.tile());
  if (qp->sparse_q)
    hipLaunchKernelGGL(k_bq_phi_sq, dim3(1), dim3(256), 0, b->stream, qp->partF, qp->gridR, qp->partP, qp->gridP, qp->partE,
                       qp->gridE, rho, eta, b->scal);
  else
    hipLaunchKernelGGL(k_bq_phi, dim3(1), dim3(256), 0, b->stream, qp->partP, qp->gridP, qp->partE, qp->gridE, rho, eta, b->scal);
  for (const StagedArg* o : {&ogx, &ogs, &oys})
    if (int rc = stage_back(b, *o)) return rc;
  if (int rc = eval_end(b, 5, &b->info.last_solve_ms)) return rc;
  *fx = b->scal_host[0];
  return FPSQ_OK;
}

int fpsq_band_qp_hprod(fpsq_band b, fpsq_band_qp qp, const double* v, double sigma, double rho, double eta,
                       int32_t hessian_approx, double* Hv) {
  if (!b || !qp || qp->b != b || !v || !Hv) return FPSQ_ERR_ARG;
  if (hessian_approx != 1 && hessian_approx != 2) {
    b->err = "band_qp_hprod: hessian_approx must be 1 or 2";
    return FPSQ_ERR_ARG;
  }
  if (int rc = eval_begin(b)) return rc;
  rho = rho > 0.0 ? rho : 0.0;
  eta = eta > 0.0 ? eta : 0.0;
  const size_t n = (size_t)b->n;
  const StagedArg av = staged(b, v, b->in_a, n);
  if (int rc = stage_in(b, av)) return rc;
  const StagedArg ah = staged(b, Hv, b->o_p1, n);
  bq_launches(b, qp, true, av.tile(), nullptr, sigma, rho, eta, ah.tile(), nullptr, nullptr);
  if (int rc = stage_back(b, ah)) return rc;
  return eval_end(b, 0, &b->info.last_solve_ms);
}

int fpsq_band_jac_mul(fpsq_band b, int32_t trans, double alpha, const double* x, double beta, double* y) {
  if (!b || !x || !y || (trans != 0 && trans != 1)) return FPSQ_ERR_ARG;
  if (!b->have_vals) {
    b->err = "band_jac_mul: the handle holds no Jacobian values yet (fpsq_band_factorize)";
    return FPSQ_ERR_STATE;
  }
  hipSetDevice(b->device);
  if (int rc = wait_input(b)) return rc;
  hipStream_t s = b->stream;
  const size_t nx = (size_t)(trans ? b->m : b->n), ny = (size_t)(trans ? b->n : b->m);
  const StagedArg ax = staged(b, x, trans ? b->in_b : b->in_a, nx);
  if (int rc = stage_in(b, ax)) return rc;
  const StagedArg ay = staged(b, y, trans ? b->o_p1 : b->o_q1, ny);
  if (beta != 0.0)  // (a staged y is an input too)
    if (int rc = stage_in(b, ay)) return rc;
  double *dx = ax.tile(), *dy = ay.tile();
  const int lg = lane_group(b->nnz, (int64_t)ny);
  if (trans && b->cols) {
    // x into the stored row order, the long columns' rows of A'x by the reduction into its virtual rows, then the product
    if (b->reordered)
      hipLaunchKernelGGL(k_gather_d, grid256(b->m), dim3(256), 0, s, dx, b->rperm, b->bd_keep, b->m);
    else
      CHK(b, hipMemcpyAsync(b->bd_keep, dx, (size_t)b->m * 8, hipMemcpyDeviceToDevice, s));
    cols_keep<1>(b, b->bd_keep);
    WITH_LANE_GROUP(lg, hipLaunchKernelGGL(k_bq_jacmul<LG>, dim3(bq_grid(b->n, lg)), dim3(256), 0, s, b->t_rowptr, b->t_colind,
                                           b->t_vals, (const int32_t*)nullptr, (const int32_t*)nullptr, alpha, b->bd_keep, beta,
                                           dy, (int)b->n))
  } else if (trans) {
    WITH_LANE_GROUP(lg, hipLaunchKernelGGL(k_bq_jacmul<LG>, dim3(bq_grid(b->n, lg)), dim3(256), 0, s, b->t_rowptr, b->t_colind,
                                           b->t_vals, b->row_perm(), (const int32_t*)nullptr, alpha, dx, beta, dy, (int)b->n))
  } else {
    WITH_LANE_GROUP(lg, hipLaunchKernelGGL(k_bq_jacmul<LG>, dim3(bq_grid(b->m, lg)), dim3(256), 0, s, b->rowptr, b->colind,
                                           b->vals, (const int32_t*)nullptr, b->row_perm(), alpha, dx, beta, dy, (int)b->m))
  }
  if (int rc = stage_back(b, ay)) return rc;
  CHK(b, hipStreamSynchronize(s));
  return FPSQ_OK;
}
}  // extern "C"

// ------- nonlinear (quadratic, separable or coupled) equality constraints on the banded handle: kernels and fpsq_band_nlp_*
#include "fpsq_band_nlp.hip.h"

// ------------------------------------------- block entries: a (k, n) block of vectors per call, 8 vectors per pass of the factor

namespace {
constexpr const char* kBlkExpired =
    "block triangular sweep: a block's solution did not arrive (bounded wait expired); the single-vector entries do not use "
    "this kernel";

// One side of a block argument, a tile of kBlkVec vectors at a time: a host-resident one goes through staging buffer `slot`
int blk_arg(fpsq_band b, const double* p, size_t len, int slot, StagedArg* a) {
  const bool host = p && !on_device(b, p);
  if (host && !b->blk_stage[slot] && dalloc(b, &b->blk_stage[slot], len * kBlkVec)) return FPSQ_ERR_HIP;
  *a = StagedArg{const_cast<double*>(p), host ? b->blk_stage[slot] : nullptr, len};
  return FPSQ_OK;
}

// the buffers a block call needs: the sweeps' own and the tiles around them
int blk_setup(fpsq_band b, bool keep, bool tv) {
  if (int rc = chain16_setup(b)) return rc;
  if (!b->blk_xg && dalloc(b, &b->blk_xg, (size_t)b->n * kBlkCols)) return FPSQ_ERR_HIP;
  if (keep && !b->blk_keep && dalloc(b, &b->blk_keep, (size_t)(b->mpad + b->vrows) * kBlkVec)) return FPSQ_ERR_HIP;
  if (tv && !b->blk_tv && dalloc(b, &b->blk_tv, (size_t)b->n * kBlkVec)) return FPSQ_ERR_HIP;
  return FPSQ_OK;
}

// the two sweeps on the tile's right-hand sides in b->r16, the border correction included: the solutions end up in b->r16
void blk_sweeps(fpsq_band b) {
  chain_sweeps16(b, b->Mb, b->band_w, b->chain_safe, b->chain_bw);
  band_correct<kBlkCols>(b, b->r16);
}

// A xg into the sweeps' layout, then the two sweeps
void blk_solve_tile(fpsq_band b, int lgA, double* keep) {
  WITH_LANE_GROUP(lgA, hipLaunchKernelGGL(k_bqb_prologue<LG>, dim3(bq_grid(b->mpad, lgA)), dim3(256), 0, b->stream, b->rowptr,
                                          b->colind, b->vals, b->blk_xg, b->r16, keep, (int)b->m, (int)b->mpad))
  if (b->cols && keep) cols_keep<kBlkVec>(b, keep);
  blk_sweeps(b);
}

// the buffers of fpsq_band_qp_objgrad_block besides blk_setup's: the partial sums, the scalars of `tiles` tiles
int og_setup(fpsq_band b, int tiles) {
  if (!b->og_scal) {
    if (dalloc(b, &b->og_partF, (size_t)kBqMaxGrid * kBlkVec) || dalloc(b, &b->og_partP, (size_t)kBqMaxGrid * kBlkCols) ||
        dalloc(b, &b->og_partE, (size_t)kBqMaxGrid * kBlkCols) || dalloc(b, &b->og_scal, (size_t)kBlkVec * 5))
      return FPSQ_ERR_HIP;
  }
  if (tiles > b->og_tiles) {
    if (b->og_scal_host) hipHostFree(b->og_scal_host);
    b->og_scal_host = nullptr;
    b->og_tiles = 0;
    CHK(b, hipHostMalloc((void**)&b->og_scal_host, (size_t)tiles * kBlkVec * 5 * 8, hipHostMallocDefault));
    b->og_tiles = tiles;
  }
  return FPSQ_OK;
}
}  // namespace

extern "C" {

int fpsq_band_solve_two_least_squares_block(fpsq_band b, int32_t k, const double* rhs1, const double* rhs2, double* p1,
                                            double* q1, double* p2, double* q2) {
  if (!b) return FPSQ_ERR_ARG;
  if (k < 1 || !rhs1 || !rhs2) {
    b->err = "band_solve_two_least_squares_block: k >= 1 and both right-hand-side blocks are required";
    return FPSQ_ERR_ARG;
  }
  if (int rc = eval_begin(b)) return rc;
  if (int rc = blk_setup(b, false, false)) return rc;
  const size_t n = (size_t)b->n, m = (size_t)b->m;
  StagedArg a1, a2, o1, oq1, o2, oq2;
  if (blk_arg(b, rhs1, n, 0, &a1) || blk_arg(b, rhs2, n, 1, &a2) || blk_arg(b, p1, n, 2, &o1) || blk_arg(b, p2, n, 3, &o2) ||
      blk_arg(b, q1, m, 4, &oq1) || blk_arg(b, q2, m, 5, &oq2))
    return FPSQ_ERR_HIP;
  const int lgA = lane_group(b->nnz, b->m), lgT = lane_group(b->nnz, b->n);
  for (int v0 = 0; v0 < k; v0 += kBlkVec) {
    const int kt = std::min<int>(kBlkVec, k - v0);
    if (int rc = stage_in(b, a1, v0, kt)) return rc;
    if (int rc = stage_in(b, a2, v0, kt)) return rc;
    hipLaunchKernelGGL(k_bqb_pack<false>, grid256(n), dim3(256), 0, b->stream, (const double*)a1.tile(v0),
                       (const double*)a2.tile(v0), (const double*)nullptr, b->blk_xg, (int)n, kt);
    blk_solve_tile(b, lgA, nullptr);
    WITH_LANE_GROUP(lgT, hipLaunchKernelGGL((k_bqb_epilogue<LG, 2>), dim3(bq_grid(b->n, lgT)), dim3(256), 0, b->stream,
                                            b->t_rowptr, b->t_colind, b->t_vals, b->r16, (const double*)nullptr, b->row_perm(),
                                            (const double*)nullptr, b->blk_xg, 0.0, 0.0, 0.0, o1.tile(v0), o2.tile(v0),
                                            oq1.tile(v0), oq2.tile(v0), (double*)nullptr, (int)n, (int)m, kt))
    for (const StagedArg* o : {&o1, &o2, &oq1, &oq2})
      if (int rc = stage_back(b, *o, v0, kt)) return rc;
  }
  return eval_end(b, 0, &b->info.last_solve_ms, kBlkExpired);
}

int fpsq_band_qp_hprod_block(fpsq_band b, fpsq_band_qp qp, int32_t k, const double* V, double sigma, double rho, double eta,
                             int32_t hessian_approx, double* HV) {
  if (!b) return FPSQ_ERR_ARG;
  if (!qp || qp->b != b || k < 1 || !V || !HV) {
    b->err = "band_qp_hprod_block: a model of this handle, k >= 1 and both blocks are required";
    return FPSQ_ERR_ARG;
  }
  if (hessian_approx != 1 && hessian_approx != 2) {
    b->err = "band_qp_hprod_block: hessian_approx must be 1 or 2";
    return FPSQ_ERR_ARG;
  }
  const size_t n = (size_t)b->n;
  {
    const uintptr_t lo = (uintptr_t)V, ho = (uintptr_t)HV, bytes = (uintptr_t)k * n * 8;
    if (lo < ho + bytes && ho < lo + bytes) {
      b->err = "band_qp_hprod_block: V and HV overlap";
      return FPSQ_ERR_ARG;
    }
  }
  if (int rc = eval_begin(b)) return rc;
  if (int rc = blk_setup(b, true, qp->sparse_q)) return rc;
  rho = rho > 0.0 ? rho : 0.0;
  eta = eta > 0.0 ? eta : 0.0;
  StagedArg av, ah;
  if (blk_arg(b, V, n, 0, &av) || blk_arg(b, HV, n, 2, &ah)) return FPSQ_ERR_HIP;
  hipStream_t s = b->stream;
  for (int v0 = 0; v0 < k; v0 += kBlkVec) {
    const int kt = std::min<int>(kBlkVec, k - v0);
    if (int rc = stage_in(b, av, v0, kt)) return rc;
    const double* dv = av.tile(v0);
    double* dh = ah.tile(v0);
    if (qp->sparse_q) {
      WITH_LANE_GROUP(qp->lgR, hipLaunchKernelGGL(k_bqb_pack_sq<LG>, dim3(qp->gridR), dim3(256), 0, s, qp->r_rowptr,
                                                  qp->r_colind, qp->r_vals, dv, qp->q, b->blk_xg, (int)n, kt))
    } else {
      hipLaunchKernelGGL(k_bqb_pack<true>, grid256(n), dim3(256), 0, s, dv, (const double*)nullptr, qp->q, b->blk_xg, (int)n,
                         kt);
    }
    blk_solve_tile(b, qp->lgA, b->blk_keep);
    WITH_LANE_GROUP(qp->lgT, WITH_BOOL(qp->sparse_q, SQ, hipLaunchKernelGGL(
        (k_bqb_epilogue<LG, SQ ? 1 : 0>), dim3(qp->gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals, b->r16,
        b->blk_keep, b->row_perm(), qp->q, b->blk_xg, sigma, rho, eta, dh, (double*)nullptr, (double*)nullptr,
        (double*)nullptr, b->blk_tv, (int)n, (int)b->m, kt)))
    if (qp->sparse_q) {
      WITH_LANE_GROUP(qp->lgR, hipLaunchKernelGGL(k_bqb_rsub<LG>, dim3(qp->gridR), dim3(256), 0, s, qp->r_rowptr, qp->r_colind,
                                                  qp->r_vals, b->blk_tv, dh, (int)n, kt))
    }
    if (int rc = stage_back(b, ah, v0, kt)) return rc;
  }
  return eval_end(b, 0, &b->info.last_solve_ms, kBlkExpired);
}

int fpsq_band_qp_objgrad_block(fpsq_band b, fpsq_band_qp qp, int32_t k, const double* X, const double* D, const double* Bv,
                               double sigma, double rho, double eta, const double* XK, double* fx, double* GX, double* YS,
                               double* GS) {
  if (!b) return FPSQ_ERR_ARG;
  if (!qp || qp->b != b || k < 1 || !X || !fx) {
    b->err = "band_qp_objgrad_block: a model of this handle, k >= 1, X and fx are required";
    return FPSQ_ERR_ARG;
  }
  const size_t n = (size_t)b->n, m = (size_t)b->m;
  {
    struct Range { const char* name; const double* p; size_t len; };
    const Range in[4] = {{"X", X, n}, {"D", D, n}, {"Bv", Bv, m}, {"XK", XK, n}};
    const Range out[3] = {{"GX", GX, n}, {"YS", YS, m}, {"GS", GS, n}};
    auto overlap = [&](const Range& u, const Range& w) {
      if (!u.p || !w.p) return false;
      const uintptr_t lo = (uintptr_t)u.p, ho = (uintptr_t)w.p;
      return lo < ho + (uintptr_t)k * w.len * 8 && ho < lo + (uintptr_t)k * u.len * 8;
    };
    for (int o = 0; o < 3; ++o) {
      for (int i = 0; i < 4 + o; ++i) {
        const Range& w = i < 4 ? in[i] : out[i - 4];
        if (overlap(out[o], w)) {
          b->err = std::string("band_qp_objgrad_block: ") + out[o].name + " and " + w.name + " overlap";
          return FPSQ_ERR_ARG;
        }
      }
    }
  }
  if (int rc = eval_begin(b)) return rc;
  if (int rc = blk_setup(b, true, qp->sparse_q)) return rc;
  const int tiles = (k + kBlkVec - 1) / kBlkVec;
  if (int rc = og_setup(b, tiles)) return rc;
  rho = rho > 0.0 ? rho : 0.0;  // (the reference adds these terms only when the parameter is positive)
  eta = eta > 0.0 ? eta : 0.0;
  StagedArg ax, ad, ab, axk, ogx, ogs, oys;
  if (blk_arg(b, X, n, 0, &ax) || blk_arg(b, D, n, 1, &ad) || blk_arg(b, GX, n, 2, &ogx) || blk_arg(b, GS, n, 3, &ogs) ||
      blk_arg(b, YS, m, 4, &oys) || blk_arg(b, Bv, m, 5, &ab) || blk_arg(b, eta > 0.0 ? XK : nullptr, n, 6, &axk))
    return FPSQ_ERR_HIP;
  hipStream_t s = b->stream;
  const double* partF = qp->sparse_q ? b->og_partF : nullptr;
  for (int v0 = 0, t = 0; v0 < k; v0 += kBlkVec, ++t) {
    const int kt = std::min<int>(kBlkVec, k - v0);
    for (const StagedArg* a : {&ax, &ad, &ab, &axk})
      if (int rc = stage_in(b, *a, v0, kt)) return rc;
    const double *dx = ax.tile(v0), *dd = ad.tile(v0), *db = ab.tile(v0), *dxk = axk.tile(v0);
    double *dgx = ogx.tile(v0), *dgs = ogs.tile(v0), *dys = oys.tile(v0);
    if (qp->sparse_q) {
      WITH_LANE_GROUP(qp->lgR, hipLaunchKernelGGL(k_bqb_og_pack_sq<LG>, dim3(qp->gridR), dim3(256), 0, s, qp->r_rowptr,
                                                  qp->r_colind, qp->r_vals, dx, dd, qp->d, qp->q, b->blk_xg, b->og_partF, (int)n,
                                                  kt))
    } else {
      hipLaunchKernelGGL(k_bqb_og_pack, grid256(n), dim3(256), 0, s, dx, dd, qp->d, qp->q, b->blk_xg, (int)n, kt);
    }
    WITH_LANE_GROUP(qp->lgA, WITH_BOOL(!qp->sparse_q, FD, hipLaunchKernelGGL(
        (k_bqb_og_prologue<LG, FD>), dim3(qp->gridP), dim3(256), 0, s, b->rowptr, b->colind, b->vals, b->blk_xg, dx, dd, qp->d,
        qp->q, db, qp->bp, b->row_perm(), b->r16, b->blk_keep, b->og_partP, (int)m, (int)b->mpad, (int)n, kt)))
    if (b->cols) cols_keep<kBlkVec>(b, b->blk_keep);
    blk_sweeps(b);
    WITH_LANE_GROUP(qp->lgT, WITH_BOOL(qp->sparse_q, SQ, hipLaunchKernelGGL(
        (k_bqb_og_epilogue<LG, SQ>), dim3(qp->gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals, b->r16, b->blk_keep,
        b->row_perm(), qp->q, b->blk_xg, dxk, sigma, rho, eta, dgx, dgs, dys, b->blk_tv, b->og_partE, (int)n, (int)m, kt)))
    if (qp->sparse_q && dgx) {  // GX -= R p2: the rows of tv are complete only now
      WITH_LANE_GROUP(qp->lgR, hipLaunchKernelGGL(k_bqb_rsub<LG>, dim3(qp->gridR), dim3(256), 0, s, qp->r_rowptr, qp->r_colind,
                                                  qp->r_vals, b->blk_tv, dgx, (int)n, kt))
    }
    hipLaunchKernelGGL(k_bqb_phi, dim3(1), dim3(256), 0, s, partF, qp->gridR, b->og_partP, qp->gridP, b->og_partE, qp->gridE, rho,
                       eta, b->og_scal);
    CHK(b, hipMemcpyAsync(b->og_scal_host + (size_t)t * kBlkVec * 5, b->og_scal, (size_t)kBlkVec * 5 * 8, hipMemcpyDeviceToHost,
                          s));
    for (const StagedArg* o : {&ogx, &ogs, &oys})
      if (int rc = stage_back(b, *o, v0, kt)) return rc;
  }
  if (int rc = eval_end(b, 0, &b->info.last_solve_ms, kBlkExpired)) return rc;
  for (int j = 0; j < k; ++j) fx[j] = b->og_scal_host[(size_t)j * 5];
  return FPSQ_OK;
}
}  // extern "C"
