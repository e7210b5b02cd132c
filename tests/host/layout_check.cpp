// layout_check.cpp -- the executable statement of what every product kernel expects to find in the arrays that
// csrc/fpsq_layout.h builds.  Stand-alone (its own main, includes nothing of the library but that header): for each
// generated case it builds every stored layout of A and A' and DECODES it the way the kernel that reads it does -- the
// decoders below restate the kernels' fetch code (k_spmv and its csort_fetch / cshared_head, the tile loop of k_spmv_rgcs,
// the flag waits of k_iter_fused), not the builders -- checking that each nonzero of the CSR comes out exactly once with
// its row, column and value source, that the padding is harmless, that every packed field is in range and that every
// index a kernel forms lies inside the array it indexes (the tail entries the kernels read unconditionally included).
// tests/test_layout_cpu.py compiles and runs it, plain and under the address / undefined-behaviour sanitizers.
#include "fpsq_layout.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

using namespace fpsq;

namespace {

int g_fail = 0;
std::string g_case;
std::set<std::string> g_branches;

void fail(const char* fmt, ...) {
  if (++g_fail > 20) return;
  std::fprintf(stderr, "FAIL [%s] ", g_case.c_str());
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
  std::fprintf(stderr, "\n");
}
#define CHECK(cond, ...) \
  do {                   \
    if (!(cond)) {       \
      fail(__VA_ARGS__); \
      return;            \
    }                    \
  } while (0)

void took(const std::string& b) {
  g_branches.insert(b);
  std::printf("  %-22s -> %s\n", g_case.c_str(), b.c_str());
}

// an index formed by a kernel: must be inside the device array (whose size is the host vector's plus `tail`)
#define INSIDE(i, vec, tail, what) CHECK((int64_t)(i) >= 0 && (int64_t)(i) < (int64_t)(vec).size() + (tail), "%s: index %lld outside %zu + %d", what, (long long)(i), (vec).size(), tail)

// ------------------------------------------------------------------------------------------------ generators (fixed seed)

uint64_t g_rng = 0;
uint32_t rnd() {  // splitmix64; every generator starts it from its own seed (tests/test_gpu_layout_branches.py draws the same)
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

HostCsr from_rows(int64_t m, int64_t n, const std::vector<std::set<int32_t>>& rows) {
  HostCsr H;
  H.nrows = m;
  H.ncols = n;
  H.rowptr.assign(1, 0);
  for (const auto& r : rows) {
    for (int32_t c : r) H.colind.push_back(c);
    H.rowptr.push_back((int32_t)H.colind.size());
  }
  return H;
}

// row i: `per` distinct columns in a window of `window` columns centred at i n / m (clamped)
std::vector<std::set<int32_t>> banded_rows(int64_t m, int64_t n, int per, int64_t window, uint64_t seed = 1) {
  g_rng = seed;
  std::vector<std::set<int32_t>> rows(m);
  for (int64_t i = 0; i < m; ++i) {
    const int64_t start = std::min(std::max<int64_t>(i * n / m - window / 2, 0), n - window);
    while ((int)rows[i].size() < per) rows[i].insert((int32_t)(start + rnd() % window));
  }
  return rows;
}

// ------------------------------------------------------------------------------------------------ decoders

struct Entry {
  int32_t row, col, src;
};
// what a product must see: every CSR entry of H once, as (row, column, value source); perm = null: the slot itself
std::vector<Entry> expected(const HostCsr& H, const std::vector<int32_t>* perm) {
  std::vector<Entry> e;
  for (int64_t r = 0; r < H.nrows; ++r)
    for (int32_t k = H.rowptr[r]; k < H.rowptr[r + 1]; ++k) e.push_back(Entry{(int32_t)r, H.colind[k], perm ? (*perm)[k] : k});
  return e;
}
void same_entries(std::vector<Entry> got, std::vector<Entry> want, const char* what) {
  auto lt = [](const Entry& a, const Entry& b) { return a.src != b.src ? a.src < b.src : a.row != b.row ? a.row < b.row : a.col < b.col; };
  std::sort(got.begin(), got.end(), lt);
  std::sort(want.begin(), want.end(), lt);
  CHECK(got.size() == want.size(), "%s: %zu entries decoded, %zu in the CSR", what, got.size(), want.size());
  for (size_t i = 0; i < got.size(); ++i)
    CHECK(got[i].row == want[i].row && got[i].col == want[i].col && got[i].src == want[i].src,
          "%s: decoded (row %d, col %d, source %d), the CSR has (row %d, col %d, source %d)", what, got[i].row, got[i].col,
          got[i].src, want[i].row, want[i].col, want[i].src);
}

// The block descriptors every k_spmv variant starts from: consecutive rows, the nonzero range of those rows, at most
// kMaxRowsPerBlk rows, at most kSpmvNnz nonzeros unless the block is ONE row.
void check_blocks(const HostCsr& H, const BlockLayout& B, int row_align) {
  const int nblk = B.nblk();
  CHECK(B.rb.size() >= 1 && B.rb[0] == 0 && B.rb[nblk] == H.nrows, "row blocks do not cover the rows");
  CHECK((int)B.blkdesc.size() == std::max(nblk, 1), "blkdesc size");
  for (int L = 0; L < nblk; ++L) {
    const BlkDesc d = B.blkdesc[L];
    CHECK(d.r0 == B.rb[L] && d.nr == B.rb[L + 1] - B.rb[L] && d.nr >= 1 && d.nr <= kMaxRowsPerBlk, "block %d: rows", L);
    CHECK(d.s == H.rowptr[d.r0] && d.e == H.rowptr[d.r0 + d.nr], "block %d: nonzero range", L);
    CHECK(d.e - d.s <= kSpmvNnz || d.nr == 1, "block %d: %d nonzeros in %d rows", L, d.e - d.s, d.nr);
    if (row_align > 1 && d.nr >= row_align && L + 1 < nblk) CHECK(d.nr % row_align == 0, "block %d: %d rows, not a multiple of %d", L, d.nr, row_align);
  }
  if (B.has_col16) {
    CHECK(B.col16.size() == H.colind.size() + 1 && (int)B.colbase.size() == nblk, "col16 / colbase sizes");
    CHECK(B.win >= 1 && B.win <= 65536, "win %d", B.win);
  }
}

// k_spmv<.., IDX16, PAD = false>: the compact CSR stream.  Value source of stored entry i: perm[i] (A': the transpose's).
void decode_stream(const HostCsr& H, const BlockLayout& B, const std::vector<int32_t>* perm, const char* what) {
  std::vector<Entry> got;
  for (int L = 0; L < B.nblk(); ++L) {
    const BlkDesc d = B.blkdesc[L];
    const int cbase = B.has_col16 ? B.colbase[L] : 0;
    auto column = [&](int ii) { return B.has_col16 ? cbase + (int)B.col16[ii] : H.colind[ii]; };
    if (d.e - d.s > kSpmvNnz) {  // one long row: every thread strides over it
      for (int i = d.s; i < d.e; ++i) got.push_back(Entry{d.r0, column(i), perm ? (*perm)[i] : i});
      continue;
    }
    for (int t = 0; t < kSpmvNnz; ++t) {
      const int i = d.s + t;
      const bool ok = i < d.e;
      const int ii = ok ? i : d.s;  // (an empty last block reads index nnz: the padding entry)
      INSIDE(ii, H.colind, 1, what);
      if (B.has_col16) INSIDE(ii, B.col16, 0, what);
      if (ii < (int)H.colind.size()) CHECK(column(ii) >= 0 && column(ii) < H.ncols, "%s: gather outside x", what);
      if (!ok) continue;  // value 0, product parked in slot t >= e - s: outside every row segment
      int rr = 0;  // phase 2: slot t belongs to the row whose segment [rowptr - s) holds it
      while (!(H.rowptr[d.r0 + rr] - d.s <= t && t < H.rowptr[d.r0 + rr + 1] - d.s)) ++rr;
      got.push_back(Entry{d.r0 + rr, column(ii), perm ? (*perm)[i] : i});
    }
  }
  same_entries(got, expected(H, perm), what);
}

// The padded layouts of k_spmv<.., PAD> (pad32 / pad16: slot = stored position), k_spmv<.., CSORT> (csort_fetch_raw /
// csort_decode) and the shared-value form (cshared_head / cshared_decode).  perm0: the value sources of the compact entries
// (what pad_blocks was given), perm: what it rewrote them to.  R (shared only): the row-group layout of A the values live in.
void decode_padded(const HostCsr& H, const BlockLayout& B, const PaddedLayout& P, const std::vector<int32_t>& perm0,
                   const std::vector<int32_t>& perm, const RgcsLayout* R, int64_t zero_pos, const char* what) {
  const int nblk = B.nblk();
  const size_t slots = (size_t)nblk * kSpmvNnz;
  CHECK(P.slots == slots, "%s: slots", what);
  const bool shared = P.kind == PadKind::shared, csort = shared || P.kind == PadKind::sorted;
  if (!shared) CHECK(perm.size() == slots, "%s: perm has %zu entries for %zu slots", what, perm.size(), slots);
  if (shared) {
    CHECK(P.nown >= 0 && perm.size() == (size_t)P.nown * kSpmvNnz, "%s: side array of %d blocks, perm %zu", what, P.nown, perm.size());
    CHECK(P.segdesc.size() == (size_t)nblk * 32 && (int)P.blkdesc.size() == nblk, "%s: descriptor sizes", what);
    CHECK(zero_pos >= 0 && zero_pos <= R->nstore && zero_pos < INT32_MAX, "%s: zero_pos", what);  // (the array has nstore + 1 entries)
  }
  std::vector<Entry> got;
  std::vector<int> rowof;
  for (int L = 0; L < nblk; ++L) {
    const BlkDesc d = B.blkdesc[L];  // (r0, nr, s: the same in the shared form, checked below)
    const int cnt = d.e - d.s;
    CHECK(cnt <= kSpmvNnz, "%s: block %d is a long row", what, L);
    const int cbase = B.has_col16 ? B.colbase[L] : 0;
    const size_t b0 = (size_t)L * kSpmvNnz;
    rowof.assign(kSpmvNnz, -1);  // phase 2: the row segments of the product buffer, from rowptr
    for (int rr = 0; rr < d.nr; ++rr)
      for (int t = H.rowptr[d.r0 + rr] - d.s; t < H.rowptr[d.r0 + rr + 1] - d.s; ++t) rowof[t] = d.r0 + rr;
    std::vector<char> hit(kSpmvNnz, 0);
    int vbase = 0;
    if (shared) {
      const BlkDesc sd = P.blkdesc[L];
      CHECK(sd.r0 == d.r0 && sd.nr == d.nr && sd.s == d.s, "%s: shared block descriptor %d", what, L);
      vbase = sd.e;
      if (vbase <= -128) CHECK(-128 - vbase < P.nown, "%s: block %d names side block %d of %d", what, L, -128 - vbase, P.nown);
    }
    for (int tid = 0; tid < kBlock; ++tid)
      for (int q = 0; q < 8; ++q) {
        int col, slot;
        int64_t src;  // the caller's value slot, -1: a stored zero
        if (!csort) {
          const size_t ii = b0 + tid + (size_t)q * kBlock;
          if (P.kind == PadKind::pad16) {
            INSIDE(ii, P.c16, 0, what);
            col = cbase + (int)P.c16[ii];
          } else {
            INSIDE(ii, P.col32, 0, what);
            col = P.col32[ii];
          }
          slot = tid + q * kBlock;
          src = perm[ii];
        } else {
          INSIDE(b0 + 8 * tid + 7, P.c16, 0, what);
          INSIDE(b0 + 8 * tid + 7, P.c8, 0, what);
          const int pk = P.c16[b0 + 8 * tid + q], hi = P.c8[b0 + 8 * tid + q];
          col = cbase + ((hi << 5) | (pk >> 11));
          slot = pk & 2047;
          CHECK(((hi << 5) | (pk >> 11)) < (1 << 13), "%s: column field", what);
          if (!shared) {  // values: double2 at [2 tid + 512 j], entry q its (q & 1) half of j = q >> 1
            const size_t vi = b0 + 2 * tid + 512 * (q >> 1) + (q & 1);
            INSIDE(vi, perm, 0, what);
            src = perm[vi];
          } else if (vbase <= -128) {  // a block with values of its own: entry t + 256 j at [2048 own + 256 j + t]
            const size_t vi = (size_t)(-128 - vbase) * kSpmvNnz + tid + (size_t)q * kBlock;
            INSIDE(vi, perm, 0, what);
            src = perm[vi];
          } else {  // lane tid % 64 of segment 4 q + tid / 64; the wave's descriptors at [32 L + 8 w, + 8)
            const int w = tid >> 6, lane = tid & 63;
            INSIDE((size_t)L * 32 + 8 * w + q, P.segdesc, 0, what);
            const SegDesc sg = P.segdesc[(size_t)L * 32 + 8 * w + q];
            const unsigned s0 = sg.w & 127u, s1 = (sg.w >> 7) & 127u, s2 = (sg.w >> 14) & 127u, nv = (sg.w >> 21) & 127u;
            CHECK(s0 <= 64 && s1 <= 64 && s2 <= 64 && nv <= 64 && (sg.w >> 28) == 0, "%s: split lanes of block %d", what, L);
            const int b0_ = (int)(sg.x & 0xffffffu), b1_ = (int)((sg.x >> 24) | ((sg.y & 0xffffu) << 8));
            const int b2_ = (int)((sg.y >> 16) | ((sg.z & 0xffu) << 16)), b3_ = (int)(sg.z >> 8);
            const int bs = (unsigned)lane < s0 ? b0_ : (unsigned)lane < s1 ? b1_ : (unsigned)lane < s2 ? b2_ : b3_;
            CHECK(bs >= 0 && bs < (1 << 24), "%s: run base", what);
            const int64_t pos = (unsigned)lane < nv ? (int64_t)vbase + bs + lane : zero_pos;
            INSIDE(pos, R->vperm, 1, what);
            src = pos < (int64_t)R->vperm.size() ? R->vperm[pos] : -1;  // (vals[nstore] is the array's zero entry)
            if ((unsigned)lane < nv) CHECK(src >= 0, "%s: a valid lane of block %d reads padding", what, L);
          }
        }
        CHECK(col >= 0 && col < H.ncols, "%s: gather of column %d outside x (block %d)", what, col, L);
        CHECK(slot >= 0 && slot < kSpmvNnz && slot < (1 << 11) && !hit[slot], "%s: slot %d of block %d taken twice", what, slot, L);
        hit[slot] = 1;
        if (src < 0) {  // padding: its zero product must land outside every row segment
          CHECK(src == -1 && rowof[slot] < 0, "%s: padding in slot %d of row %d", what, slot, rowof[slot]);
          continue;
        }
        CHECK(rowof[slot] >= 0, "%s: a value in slot %d outside the rows of block %d", what, slot, L);
        // the shared form reads A's value through the row groups: the source is a CSR slot of A, as perm0 names it
        got.push_back(Entry{rowof[slot], col, (int32_t)src});
      }
  }
  same_entries(got, expected(H, &perm0), what);
}

// k_spmv_rgcs (rgcs_group): fetch_stream / fetch_segs, the tile loop
void decode_rgcs(const HostCsr& H, const RgcsLayout& R, const char* what) {
  const int ng = (int)R.groups.size();
  const int stride = R.padded ? R.budget : 0;
  CHECK((int64_t)R.pidx.size() == R.nstore && (int64_t)R.vperm.size() == R.nstore, "%s: nstore", what);
  CHECK((int)R.col_range.size() == ng, "%s: col_range", what);
  if (R.padded) CHECK(R.budget % kRgcsTile == 0 && R.budget >= kRgcsTile && R.nstore == (int64_t)ng * R.budget, "%s: budget", what);
  std::vector<Entry> got;
  int next_row = 0;
  for (int g = 0; g < ng; ++g) {
    const RgcsGroup gd = R.groups[g];
    CHECK(gd.r0 == next_row && gd.R >= 1 && gd.R <= kRgcsMaxRows, "%s: rows of group %d", what, g);
    next_row += gd.R;
    const bool PAD = stride > 0;
    const int e0 = PAD ? g * stride : gd.e0, e1 = PAD ? g * stride + (gd.e1 - gd.e0) : gd.e1;
    CHECK(gd.e1 >= gd.e0 && (!PAD || gd.e1 - gd.e0 <= stride), "%s: entries of group %d", what, g);
    // the first tile's stream and segments are requested whatever the group holds
    if (PAD) INSIDE(g * (int64_t)stride + kRgcsTile - 1, R.pidx, 1, what);
    INSIDE(gd.tp + gd.R, R.tptr, 2, what);
    int tile = 0;
    for (int base = e0; base < e1; base += kRgcsTile, ++tile) {
      const int64_t tpt = gd.tp + (int64_t)tile * (gd.R + 1);
      INSIDE(tpt + gd.R, R.tptr, 0, what);  // (rows rq and rq + 1 in one 4-byte read)
      for (int rr = 0; rr < gd.R; ++rr) CHECK(R.tptr[tpt + rr] <= R.tptr[tpt + rr + 1], "%s: tptr decreases", what);
      CHECK(R.tptr[tpt + gd.R] <= kRgcsTile, "%s: tptr past the tile", what);
      std::vector<char> hit(kRgcsTile, 0);
      for (int t = 0; t < kRgcsTile; ++t) {
        const int i = base + t;
        const int ii = PAD ? i : (i < e1 ? i : e0);
        INSIDE(ii, R.pidx, 1, what);
        const bool ok = PAD || i < e1;
        const uint32_t pq = ok ? R.pidx[ii] : ((uint32_t)t << kRgcsColBits);
        const int64_t src = ok ? R.vperm[ii] : -1;
        const int col = gd.cmin + (int)(pq & ((1u << kRgcsColBits) - 1));
        const int slot = (int)(pq >> kRgcsColBits);
        CHECK(col >= 0 && col < H.ncols, "%s: gather of column %d outside x (group %d)", what, col, g);
        CHECK(slot < kRgcsTile && slot < (1 << 11) && !hit[slot], "%s: slot %d of group %d tile %d taken twice", what, slot, g, tile);
        hit[slot] = 1;
        int rr = 0;
        while (rr < gd.R && !(R.tptr[tpt + rr] <= slot && slot < R.tptr[tpt + rr + 1])) ++rr;
        if (src < 0) {
          CHECK(src == -1 && rr == gd.R, "%s: padding in a row segment (group %d)", what, g);
          continue;
        }
        CHECK(PAD ? i < e1 : true, "%s: a value behind the group's entries", what);
        CHECK(rr < gd.R, "%s: a value outside the row segments (group %d)", what, g);
        got.push_back(Entry{gd.r0 + rr, col, (int32_t)src});
      }
    }
    if (PAD)  // what lies behind the last tile of a padded group is never read as a value: it must not name one
      for (int64_t i = e0 + (int64_t)tile * kRgcsTile; i < (int64_t)(g + 1) * stride; ++i) CHECK(R.vperm[i] == -1, "%s: value behind the tiles", what);
    CHECK(R.col_range[g].x == gd.cmin && R.col_range[g].y >= gd.cmin && R.col_range[g].y - gd.cmin < (1 << kRgcsColBits), "%s: col_range", what);
  }
  CHECK(next_row == H.nrows, "%s: groups do not cover the rows", what);
  same_entries(got, expected(H, nullptr), what);
  if (R.padded) {
    CHECK(R.csr_pos.size() == H.colind.size(), "%s: csr_pos", what);
    for (size_t k = 0; k < R.csr_pos.size(); ++k)
      CHECK(R.csr_pos[k] >= 0 && R.csr_pos[k] < R.nstore && R.vperm[R.csr_pos[k]] == (int32_t)k, "%s: csr_pos[%zu]", what, k);
  }
}

// The waits of the one-launch iteration: row group g gathers 16-byte rows of the long pair at agent scope, i.e. whole
// 128-byte lines (8 rows); the A' block that writes ANY row of a line it reads must have been waited for, and vice versa.
void check_dependence(const HostCsr& HA, const BlockLayout& BT, const RgcsLayout& R, int64_t ovl, int64_t ovr, int halo_gf) {
  const int64_t n = HA.ncols;
  const int nblk = BT.nblk(), ng = (int)R.groups.size();
  CHECK(rowblocks_aligned(BT.rb, 8), "dependence tables need A' blocks on 8-row boundaries");
  const std::vector<Range2> dep = fused_dep(BT.rb, R.col_range, n);
  const std::vector<Range2> bdep = fused_bdep(dep, nblk);
  const HaloDep hd = fused_halo_dep(BT.rb, R.col_range, n, ovl, ovr, halo_gf);
  CHECK((int)dep.size() == ng && (int)bdep.size() == nblk && (int)hd.dep2.size() == ng, "dependence table sizes");
  std::vector<int> owner(n);
  for (int L = 0; L < nblk; ++L)
    for (int r = BT.rb[L]; r < BT.rb[L + 1]; ++r) owner[r] = L;
  std::vector<char> gathered(nblk, 0);
  for (int g = 0; g < ng; ++g) {
    CHECK(dep[g].x >= 0 && dep[g].y < nblk, "dep[%d] outside the flags", g);
    bool touches = false;
    const RgcsGroup gd = R.groups[g];
    for (int r = gd.r0; r < gd.r0 + gd.R; ++r)
      for (int k = HA.rowptr[r]; k < HA.rowptr[r + 1]; ++k) {
        const int64_t c = HA.colind[k];
        for (int64_t row = c & ~7ll; row <= std::min<int64_t>(c | 7, n - 1); ++row) {
          const int L = owner[row];
          gathered[L] = 1;
          CHECK(dep[g].x <= L && L <= dep[g].y, "group %d gathers from block %d, waits for [%d, %d]", g, L, dep[g].x, dep[g].y);
          CHECK(bdep[L].x <= g && g <= bdep[L].y, "block %d is gathered by group %d, waits for [%d, %d]", L, g, bdep[L].x, bdep[L].y);
        }
      }
    // dep2: exactly the groups whose line-rounded column window reaches an overlap region wait for the finish workgroups
    for (int64_t row = R.col_range[g].x & ~7ll; row <= std::min<int64_t>(R.col_range[g].y | 7, n - 1); ++row)
      touches = touches || row < ovl || row >= n - ovr;
    if (touches) CHECK(hd.dep2[g].x == nblk && hd.dep2[g].y == nblk + halo_gf - 1, "dep2[%d] not set", g);
    else CHECK(hd.dep2[g].y < hd.dep2[g].x, "dep2[%d] set for a group that touches no overlap region", g);
  }
  for (int L = 0; L < nblk; ++L) {
    CHECK(bdep[L].x >= 0 && bdep[L].y < ng, "bdep[%d] outside the flags", L);
    bool any = gathered[L];
    for (int g = 0; g < ng && !any; ++g) any = dep[g].x <= L && L <= dep[g].y;  // (the cover by one range may reach it)
    if (!any) CHECK(bdep[L].x == 0 && bdep[L].y == ng - 1, "block %d (gathered by nobody) does not wait for all groups", L);
  }
  // the blocks that deposit raw sums of the overlap regions
  for (int64_t row = 0; row < n; ++row) {
    if (row < ovl) CHECK(hd.depL.x <= owner[row] && owner[row] <= hd.depL.y, "depL misses block %d", owner[row]);
    if (row >= n - ovr) CHECK(hd.depR.x <= owner[row] && owner[row] <= hd.depR.y, "depR misses block %d", owner[row]);
  }
  if (ovl == 0) CHECK(hd.depL.y < hd.depL.x, "depL not empty");
  if (ovr == 0) CHECK(hd.depR.y < hd.depR.x, "depR not empty");
  took("dependence");
}

// ------------------------------------------------------------------------------------------------ one case, as finish_structure does it

const char* kind_name(PadKind k) {
  switch (k) {
    case PadKind::none: return "declined";
    case PadKind::pad32: return "pad32";
    case PadKind::pad16: return "pad16";
    case PadKind::sorted: return "sorted";
    case PadKind::shared: return "shared";
  }
  return "?";
}

struct Switches {
  int row_align = 8;
  bool allow_col16 = true, want_sorted = true, want_shared = true, phase_order = true;
  int tiles = 0, cus = 256;
};

void run_case(const std::string& name, const HostCsr& HA, const Switches& sw = {}) {
  g_case = name;
  const int before = g_fail;
  HostCsr HT;
  std::vector<int32_t> permT;
  transpose_structure(HA, HT, permT);
  {  // the transpose itself
    std::vector<Entry> got;
    for (int64_t r = 0; r < HT.nrows; ++r)
      for (int k = HT.rowptr[r]; k < HT.rowptr[r + 1]; ++k) got.push_back(Entry{HT.colind[k], (int32_t)r, permT[k]});
    same_entries(got, expected(HA, nullptr), "transpose");
  }
  // the row groups of A
  const RgcsLayout R = build_rgcs(HA, sw.cus, sw.tiles, sw.phase_order);
  if (R.ok) {
    decode_rgcs(HA, R, "row groups of A");
    took(std::string("rgcs ") + (R.padded ? "padded" : "compact") + (sw.phase_order ? "" : ", plain column order"));
  } else {
    took("rgcs not built");
  }
  // both matrices: the compact stream, then every padded form it can be re-stored in
  for (int side = 0; side < 2; ++side) {
    const HostCsr& H = side ? HT : HA;
    const std::string who = side ? "A'" : "A";
    const int align = side ? sw.row_align : 1;
    const BlockLayout B = build_blocks(H, align, sw.allow_col16);
    check_blocks(H, B, align);
    if (side && align == 8 && rowblocks_aligned(B.rb, 8)) took("A' blocks on 8-row lines");
    decode_stream(H, B, side ? &permT : nullptr, (who + " stream").c_str());
    took(who + (B.has_col16 ? " stream col16" : " stream 32-bit columns"));
    std::vector<int32_t> ident(H.colind.size());
    for (size_t k = 0; k < ident.size(); ++k) ident[k] = (int32_t)k;
    const std::vector<int32_t>& perm0 = side ? permT : ident;
    for (int share = 0; share < 2; ++share) {
      // (share = 1: what the library does for A' when the row groups are padded; share = 0: FPSQ_AT_SHARED=0 / no row groups)
      if (share && !(side && R.ok && R.padded)) continue;
      std::vector<int32_t> perm = perm0;
      const PaddedLayout P = pad_blocks(H, B, perm, sw.want_sorted, share && sw.want_shared, share ? &R.csr_pos : nullptr, R.nstore);
      if (P.kind == PadKind::none) {
        CHECK(perm == perm0, "pad_blocks declined but rewrote perm");
        bool longrow = H.colind.empty();
        for (int L = 0; L < B.nblk(); ++L) longrow = longrow || B.blkdesc[L].e - B.blkdesc[L].s > kSpmvNnz;
        CHECK(longrow, "pad_blocks declined without a long row");
        took(who + " pad declined");
        continue;
      }
      decode_padded(H, B, P, perm0, perm, &R, R.nstore, (who + " " + kind_name(P.kind)).c_str());
      took(who + " " + kind_name(P.kind));
      if (P.kind == PadKind::shared && P.nown > 0) took("shared with own blocks");
      if (P.kind == PadKind::shared && P.nown == 0) took("shared, no own blocks");
      if (P.kind != PadKind::shared && P.nown >= 0) took("shared rejected");
    }
    if (side && R.ok && R.padded && rowblocks_aligned(B.rb, 8)) {
      const int64_t n = HA.ncols;
      check_dependence(HA, B, R, 0, 0, 0);
      if (n >= 64) check_dependence(HA, B, R, n / 8 / 8 * 8, (n - (n - n / 16) / 8 * 8), 3);
    }
  }
  std::printf("%-24s m=%lld n=%lld nnz=%zu: %s\n", name.c_str(), (long long)HA.nrows, (long long)HA.ncols, HA.colind.size(),
              g_fail == before ? "ok" : "FAILED");
}

}  // namespace

int main() {
  // banded: sorted + shared
  run_case("banded", from_rows(512, 4096, banded_rows(512, 4096, 12, 256)));
  {
    Switches s;
    s.row_align = 1;
    run_case("banded align 1", from_rows(512, 4096, banded_rows(512, 4096, 12, 256)), s);
    s = Switches{};
    s.allow_col16 = false;  // jac_format = 1
    run_case("banded no col16", from_rows(512, 4096, banded_rows(512, 4096, 12, 256)), s);
    s = Switches{};
    s.phase_order = false;
    run_case("banded plain order", from_rows(512, 4096, banded_rows(512, 4096, 12, 256)), s);
    s = Switches{};
    s.want_sorted = false;
    run_case("banded row order", from_rows(512, 4096, banded_rows(512, 4096, 12, 256)), s);
    s = Switches{};
    s.tiles = 3;
    s.cus = 4;
    run_case("banded 4 CUs", from_rows(512, 4096, banded_rows(512, 4096, 12, 256)), s);
  }
  // the same rows in a window of 20000 columns: blocks of A wider than 8192 columns (16-bit columns, not sortable)
  run_case("window 20000", from_rows(512, 40000, banded_rows(512, 40000, 12, 20000)));
  // ... and an A' like that (tests/structures.py "wide-window"): what the library pads
  {
    const int m = 10000, n = 12000;
    std::vector<std::set<int32_t>> rows(m);
    for (int64_t i = 0; i < m; ++i) rows[i] = {(int32_t)i, (int32_t)(i * 7919 % n), (int32_t)((i * 104729 + 13) % n)};
    run_case("wide A'", from_rows(m, n, rows));
  }
  // columns uniform over 200000: a block of A spans more than 65535 columns
  run_case("uniform 200000", from_rows(512, 200000, banded_rows(512, 200000, 12, 200000)));
  {  // one row of 3000 entries: longer than an LDS stage and than a row group's budget
    std::vector<std::set<int32_t>> rows(1);
    g_rng = 1;
    while (rows[0].size() < 3000) rows[0].insert((int32_t)(rnd() % 4000));
    run_case("one long row", from_rows(1, 4000, rows));
  }
  {  // empty rows and empty columns
    std::vector<std::set<int32_t>> rows = banded_rows(300, 600, 5, 600);
    for (int i = 0; i < 300; i += 7) rows[i].clear();
    rows[299].clear();
    run_case("empty rows/columns", from_rows(300, 5000, rows));
  }
  {
    std::vector<std::set<int32_t>> rows(1);
    rows[0] = {0, 1, 2};
    run_case("m = 1", from_rows(1, 3, rows));
    std::vector<std::set<int32_t>> none(4);
    run_case("no entries", from_rows(4, 16, none));
  }
  {  // Every 16th row also reaches into the first eight columns: the first block of A' then collects, from every row group,
     // a handful of entries that sit apart in the group's sorted order -- more than four runs in a 64-entry segment.
    const int m = 1024, n = 8192;
    std::vector<std::set<int32_t>> rows = banded_rows(m, n, 12, 256);
    for (int i = 0; i < m; i += 16) rows[i].insert((i / 16) % 8);
    run_case("piled first block", from_rows(m, n, rows));
  }
  // two entries per row anywhere: each of the 32 blocks of A' collects eight entries from every one of 64 row groups -- eight
  // runs in a 64-entry segment, every block would keep its own values, and the shared form is given up for the sorted one
  run_case("scattered", from_rows(8192, 32768, banded_rows(8192, 32768, 2, 32768)));
  {  // a group wider than 2^21 columns: no row groups
    std::vector<std::set<int32_t>> rows(2);
    rows[0] = {0, 2200000};
    rows[1] = {5};
    run_case("span 2^21", from_rows(2, 2200001, rows));
  }
  const char* must[] = {"A' sorted", "A' shared", "A pad16", "A' pad16", "A stream 32-bit columns", "A pad declined", "A' pad32",
                        "A pad32", "rgcs padded", "rgcs compact", "rgcs padded, plain column order", "rgcs not built",
                        "shared with own blocks", "shared rejected", "A' blocks on 8-row lines", "dependence", "A' stream col16"};
  for (const char* b : must)
    if (!g_branches.count(b)) {
      std::fprintf(stderr, "FAIL: no case reached the branch \"%s\"\n", b);
      ++g_fail;
    }
  std::printf("%d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}
