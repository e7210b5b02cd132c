// fpsq_layout.h -- everything the product kernels read from the Jacobian, ENCODED ON THE HOST: the constants and descriptor
// structs the host and the kernels must agree on, and the builders of every stored layout (row blocks, 16-bit columns, padded /
// column-sorted / shared-value blocks of A', the row-group copy of A, the dependence ranges of the one-launch iteration).
// Plain C++17: no device runtime, no solver state, no environment, no allocation but std::vector -- the builders return host
// data and the library's host side uploads it, so all of this index arithmetic runs (and is checked: tests/host/layout_check.cpp decodes
// every layout the way the kernel that reads it does) without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace fpsq {

// ------------------------------------------------------------------------------------------------ shared constants

constexpr int kBlock = 256;        // threads per workgroup (4 waves)
static_assert(kBlock == 256, "block_sum / block_sum_lanes and the tile-per-thread constants assume 4 waves");
#ifndef FPSQ_SPMV_NNZ
#define FPSQ_SPMV_NNZ 2048
#endif
constexpr int kSpmvNnz = FPSQ_SPMV_NNZ;  // nonzeros staged through LDS per workgroup
constexpr int kMaxRowsPerBlk = 1024;
constexpr int kEwBlocksMax = 1024; // grid cap for element-wise kernels (grid-stride beyond)
static_assert(kSpmvNnz <= 2048, "slot field of the column-sorted layout is 11 bits");

#ifndef FPSQ_RGCS_TILE
#define FPSQ_RGCS_TILE 2048
#endif
#ifndef FPSQ_RGCS_GROUP_NNZ
#define FPSQ_RGCS_GROUP_NNZ 12800
#endif
#ifndef FPSQ_RGCS_MAX_ROWS
#define FPSQ_RGCS_MAX_ROWS 128
#endif
constexpr int kRgcsTile = FPSQ_RGCS_TILE;
constexpr int kRgcsColBits = 21;     // group-relative column < 2^21, slot < 2^11
constexpr int kRgcsGroupNnz = FPSQ_RGCS_GROUP_NNZ;
constexpr int kRgcsMaxRows = FPSQ_RGCS_MAX_ROWS;
static_assert(kRgcsTile <= 2048 && kRgcsTile % kBlock == 0, "slot field is 11 bits");

struct RgcsGroup {        // 32 bytes, fetched with two independent 16-byte loads at the head of the workgroup
  int32_t r0, R;          // first row, #rows
  int32_t e0, e1;         // entry range
  int32_t cmin;           // smallest column of the group
  int32_t tp;             // offset into tptr
  int32_t pad[2];
};

// Host images of the device arrays the kernels read through vector types: same size, same field order (the upload functions
// assert the sizes).
struct BlkDesc {  // CsrView::blkdesc (int4): {first row, #rows, first nonzero, end nonzero -- or the value base of a shared block}
  int32_t r0, nr, s, e;
};
struct SegDesc {  // CsrView::segdesc (uint4): four 24-bit run bases, three 7-bit split lanes, the number of valid lanes
  uint32_t x, y, z, w;
};
struct Range2 {   // an inclusive range (int2); {1, 0} is the empty one
  int32_t x, y;
};

// ------------------------------------------------------------------------------------------------ CSR, row blocks, transpose

struct HostCsr {
  int64_t nrows, ncols;
  std::vector<int32_t> rowptr, colind;
};

// align > 1 (the A' blocks of a solver whose iterations run as one launch, k_iter_fused): a block that holds at least `align` rows
// ends on a multiple of `align` rows -- with 16-byte rows of the long pair and align = 8 every 128-byte line of the product's
// output then belongs to ONE block.  (Blocks of fewer rows -- very long rows -- stay as they are: rowblocks_aligned() says so.)
inline std::vector<int32_t> make_rowblocks(const std::vector<int32_t>& rowptr, int64_t nrows, int align = 1) {
  std::vector<int32_t> rb;
  rb.push_back(0);
  int64_t r = 0;
  while (r < nrows) {
    int64_t r1 = r;
    int64_t nz = 0;
    while (r1 < nrows && (r1 - r) < kMaxRowsPerBlk) {
      const int64_t len = rowptr[r1 + 1] - rowptr[r1];
      if (nz + len > kSpmvNnz) break;
      nz += len;
      ++r1;
    }
    if (r1 == r) r1 = r + 1;  // a single row longer than kSpmvNnz gets a block of its own
    else if (align > 1 && r1 < nrows && r1 - r >= align) r1 = r + (r1 - r) / align * align;
    rb.push_back((int32_t)r1);
    r = r1;
  }
  return rb;
}

inline bool rowblocks_aligned(const std::vector<int32_t>& rb, int align) {
  for (size_t i = 0; i + 1 < rb.size(); ++i)
    if (rb[i] % align) return false;
  return true;
}

// transpose structure: returns CSR of A' and perm with AT slot t <- A slot perm[t]
inline void transpose_structure(const HostCsr& A, HostCsr& T, std::vector<int32_t>& perm) {
  const int64_t nnz = (int64_t)A.colind.size();
  T.nrows = A.ncols;
  T.ncols = A.nrows;
  T.rowptr.assign(T.nrows + 1, 0);
  for (int64_t k = 0; k < nnz; ++k) T.rowptr[A.colind[k] + 1]++;
  for (int64_t j = 0; j < T.nrows; ++j) T.rowptr[j + 1] += T.rowptr[j];
  T.colind.resize(nnz);
  perm.resize(nnz);
  std::vector<int32_t> next(T.rowptr.begin(), T.rowptr.end() - 1);
  for (int64_t i = 0; i < A.nrows; ++i)
    for (int32_t k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k) {
      const int32_t t = next[A.colind[k]]++;
      T.colind[t] = (int32_t)i;
      perm[t] = k;
    }
}

// ------------------------------------------------------------------------------------------------ row blocks of k_spmv

struct BlockLayout {
  std::vector<int32_t> rb;        // nblk + 1 row boundaries
  std::vector<BlkDesc> blkdesc;   // max(nblk, 1) descriptors
  // 16-bit block-relative columns (has_col16): col = colbase[block] + col16[k]; one padding entry behind the nnz
  bool has_col16 = false;
  std::vector<uint16_t> col16;
  std::vector<int32_t> colbase;
  int32_t win = 0;                // with col16: widest column span of a row block
  int nblk() const { return (int)rb.size() - 1; }
};

inline BlockLayout build_blocks(const HostCsr& H, int row_align, bool allow_col16) {
  BlockLayout B;
  const int64_t nnz = (int64_t)H.colind.size();
  B.rb = make_rowblocks(H.rowptr, H.nrows, row_align);
  const std::vector<int32_t>& rb = B.rb;
  const int nblk = B.nblk();
  B.blkdesc.resize(std::max(nblk, 1));
  for (int b = 0; b < nblk; ++b) B.blkdesc[b] = BlkDesc{rb[b], rb[b + 1] - rb[b], H.rowptr[rb[b]], H.rowptr[rb[b + 1]]};
  // 16-bit block-relative columns when every row block spans < 65536 columns
  if (allow_col16 && nnz > 0) {
    std::vector<int32_t> base(nblk, 0);
    std::vector<uint16_t> c16(nnz + 1, 0);
    bool ok = true;
    int span = 0;
    for (int b = 0; b < nblk && ok; ++b) {
      const int s = H.rowptr[rb[b]], e = H.rowptr[rb[b + 1]];
      int lo = INT32_MAX, hi = -1;
      for (int k = s; k < e; ++k) {
        lo = std::min(lo, H.colind[k]);
        hi = std::max(hi, H.colind[k]);
      }
      if (e == s) lo = hi = 0;
      if (hi - lo > 65535) ok = false;
      span = std::max(span, hi - lo + 1);
      base[b] = lo;
      for (int k = s; k < e && ok; ++k) c16[k] = (uint16_t)(H.colind[k] - lo);
    }
    if (ok) {
      B.has_col16 = true;
      B.col16.swap(c16);
      B.colbase.swap(base);
      B.win = span;
    }
  }
  return B;
}

// ------------------------------------------------------------------------------------------------ padded blocks of k_spmv

enum class PadKind { none, pad32, pad16, sorted, shared };

struct PaddedLayout {
  PadKind kind = PadKind::none;
  size_t slots = 0;               // nblk * kSpmvNnz
  std::vector<int32_t> col32;     // pad32: the columns
  std::vector<uint16_t> c16;      // pad16: block-relative columns; sorted / shared: slot | (col & 31) << 11
  std::vector<uint8_t> c8;        // sorted / shared: col >> 5
  // shared: one descriptor per 64 stored entries, and the block descriptors with the value base (or -128 - i for the i-th
  // block that keeps values of its own) in the place of the end nonzero
  std::vector<SegDesc> segdesc;
  std::vector<BlkDesc> blkdesc;
  int nown = -1;                  // blocks that keep their own values, counted when the shared layout was tried (-1: not tried)
};

// Re-store a CSR in the padded block layout of k_spmv<.., PAD>.  `perm` (value source of every compact entry)
// is rewritten to the padded numbering with -1 in the padding slots.  Not padded when some block is one long row.
// csr_pos (optional, A' only): for every CSR slot of A its position in the padded row-group copy of A (build_rgcs), and
// zero_pos, a position of that array that always holds 0.0.  When given -- and the blocks qualify for the column-sorted
// layout -- the blocks are stored WITHOUT VALUES: an A' block's entries come from the ~10 row groups whose column windows
// reach its columns, and inside a group (column-sorted) they are a contiguous run; the block's entries are therefore
// stored in the order of their POSITIONS in the row-group array, 64 consecutive entries (one wave instruction) read at most
// four runs, and one 16-byte descriptor per such segment says where: four 24-bit bases relative to the block's base
// (blkdesc.w), three split lanes, the number of valid lanes.  The index planes keep the column-sorted format (slot in the
// block's row-major order | column relative to colbase), so the products land in the same LDS slots and are summed in the
// same order: BITWISE the other layouts.  What it buys: the Krylov loop streams ONE copy of the values (80 MB less
// working set next to a 256 MB Infinity Cache: measured as a what-if in round 3, +3.9 % evaluations/s at the headline
// size), a Jacobian refresh writes one array instead of two, 82 MB less memory.  The value addresses need the descriptors
// first -- but so do the gathers of x need the index words, and values and gathers then travel in the same round trip: the
// workgroup's chain of dependent memory round trips is no longer.
inline PaddedLayout pad_blocks(const HostCsr& H, const BlockLayout& B, std::vector<int32_t>& perm, bool want_sorted,
                               bool want_shared, const std::vector<int32_t>* csr_pos = nullptr, int64_t zero_pos = 0) {
  PaddedLayout P;
  if (H.colind.empty()) return P;
  const std::vector<int32_t>& rb = B.rb;
  const int nblk = B.nblk();
  for (int b = 0; b < nblk; ++b)
    if (H.rowptr[rb[b + 1]] - H.rowptr[rb[b]] > kSpmvNnz) return P;
  const size_t slots = (size_t)nblk * kSpmvNnz;
  if (slots >= (size_t)INT32_MAX) return P;
  P.slots = slots;
  std::vector<int32_t> pperm(slots, -1), pcol;
  std::vector<uint16_t> pc16;
  std::vector<uint8_t> pc8;
  std::vector<int32_t> ord;
  const std::vector<int32_t>& base = B.colbase;
  const bool idx16 = B.has_col16;
  // column-sorted blocks (k_spmv<.., CSORT>): 13 bits of block-relative column next to the 11-bit slot
  const bool sorted = idx16 && B.win <= 8192 && want_sorted;
  if (sorted) {
    pc16.resize(slots);
    for (size_t q = 0; q < slots; ++q) {  // padding: an unused slot (its own sorted position), column 0, value 0
      const size_t t = q % kSpmvNnz;
      pc16[q - t + 8 * ((t % 512) / 2) + 2 * (t / 512) + (t & 1)] = (uint16_t)t;
    }
    pc8.assign(slots, 0);
  } else if (idx16) {
    pc16.assign(slots, 0);
  } else {
    pcol.assign(slots, 0);
  }
  // ---- shared values.  A block whose entries cannot be described that way (a 64-entry segment touching more than four
  // runs: the first blocks of the headline generators, where the clamped windows of the top rows pile several groups' last
  // few columns into one block) keeps 2048 values of its OWN in a small side array (refreshed like before); its
  // blkdesc.w = -128 - (its index there) tells the kernel.  More than a quarter of the blocks like that: not worth it.
  bool shared = sorted && csr_pos != nullptr && want_shared && zero_pos < (int64_t)INT32_MAX;
  std::vector<SegDesc> segd;
  std::vector<int32_t> vbase, own_perm;
  std::vector<uint16_t> sc16;
  std::vector<uint8_t> sc8;
  int nown = 0;
  if (shared) {
    segd.assign((size_t)nblk * 32, SegDesc{0u, 0u, 0u, 0u});
    vbase.assign(nblk, 0);
    sc16.resize(slots);
    sc8.assign(slots, 0);
    std::vector<int64_t> pos;
    std::vector<SegDesc> sd(32);
    for (int b = 0; b < nblk; ++b) {
      const int s = H.rowptr[rb[b]], e = H.rowptr[rb[b + 1]], cnt = e - s;
      ord.resize(cnt);
      pos.resize(cnt);
      for (int k = 0; k < cnt; ++k) {
        ord[k] = k;
        pos[k] = (*csr_pos)[perm[s + k]];
      }
      std::sort(ord.begin(), ord.end(), [&](int a, int c) { return pos[a] < pos[c]; });
      const int64_t base64 = (cnt ? pos[ord[0]] : 0) - 64;
      bool ok = true;
      for (int sg = 0; sg < 32 && ok; ++sg) {
        const int lo = sg * 64, nvalid = std::max(0, std::min(64, cnt - lo));
        int64_t vb[4] = {0, 0, 0, 0};
        int split[3] = {64, 64, 64};
        int np = 0;
        for (int l = 0; l < nvalid && ok; ++l) {
          const int64_t p = pos[ord[lo + l]];
          if (l == 0 || p != pos[ord[lo + l - 1]] + 1) {  // a new run starts at lane l
            if (np == 4) {
              ok = false;
              break;
            }
            if (np > 0) split[np - 1] = l;
            vb[np++] = p - l - base64;
          }
        }
        for (int i = 0; i < 4; ++i)
          if (vb[i] < 0 || vb[i] >= (1ll << 24)) ok = false;
        const uint64_t a0 = (uint64_t)vb[0] | ((uint64_t)vb[1] << 24) | ((uint64_t)vb[2] << 48);
        SegDesc d;
        d.x = (uint32_t)a0;
        d.y = (uint32_t)(a0 >> 32);
        d.z = (uint32_t)(((uint64_t)vb[2] >> 16) | ((uint64_t)vb[3] << 8));
        d.w = (uint32_t)split[0] | ((uint32_t)split[1] << 7) | ((uint32_t)split[2] << 14) | ((uint32_t)nvalid << 21);
        sd[(sg % 4) * 8 + sg / 4] = d;  // (stored per wave: segment 4 j + w at [8 w + j], a wave's eight in one 128-byte line)
      }
      if (ok) {
        vbase[b] = (int32_t)base64;
        for (int sg = 0; sg < 32; ++sg) segd[(size_t)b * 32 + sg] = sd[sg];
      } else {  // its own values, in column-sorted order
        vbase[b] = -128 - nown;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int c) { return H.colind[s + a] < H.colind[s + c]; });
        own_perm.resize((size_t)(nown + 1) * kSpmvNnz, -1);
        for (int t = 0; t < cnt; ++t) own_perm[(size_t)nown * kSpmvNnz + t] = perm[s + ord[t]];
        ++nown;
      }
      for (int t = 0; t < kSpmvNnz; ++t) {  // entry t of the stored order belongs to thread t % 256, its j-th word (j = t / 256)
        const size_t qi = (size_t)b * kSpmvNnz + 8 * (t % kBlock) + t / kBlock;
        if (t < cnt) {
          const int k = ord[t], col = H.colind[s + k] - base[b];
          sc16[qi] = (uint16_t)(k | ((col & 31) << 11));
          sc8[qi] = (uint8_t)(col >> 5);
        } else {
          sc16[qi] = (uint16_t)t;  // an unused slot of the product buffer; its value is 0 (zero_pos / the side array's padding)
        }
      }
    }
    P.nown = nown;
    if (nown > nblk / 4) shared = false;
  }
  if (shared) {
    P.kind = PadKind::shared;
    P.c16.swap(sc16);
    P.c8.swap(sc8);
    P.segdesc.swap(segd);
    P.blkdesc.resize(nblk);
    for (int b = 0; b < nblk; ++b) P.blkdesc[b] = BlkDesc{rb[b], rb[b + 1] - rb[b], H.rowptr[rb[b]], vbase[b]};
    perm.swap(own_perm);
    return P;
  }
  for (int b = 0; b < nblk; ++b) {
    const int s = H.rowptr[rb[b]], e = H.rowptr[rb[b + 1]];
    if (sorted) {
      ord.resize(e - s);
      for (int k = s; k < e; ++k) ord[k - s] = k;
      std::stable_sort(ord.begin(), ord.end(), [&](int a, int c) { return H.colind[a] < H.colind[c]; });
      for (int t = 0; t < e - s; ++t) {
        const int k = ord[t], col = H.colind[k] - base[b];
        const size_t q = (size_t)b * kSpmvNnz + t;
        pperm[q] = perm[k];
        // (index planes: the eight entries of a thread contiguously, see csort_fetch)
        const size_t qi = (size_t)b * kSpmvNnz + 8 * ((t % 512) / 2) + 2 * (t / 512) + (t & 1);
        pc16[qi] = (uint16_t)((k - s) | ((col & 31) << 11));
        pc8[qi] = (uint8_t)(col >> 5);
      }
      continue;
    }
    for (int k = s; k < e; ++k) {
      const size_t q = (size_t)b * kSpmvNnz + (k - s);
      pperm[q] = perm[k];
      if (idx16) pc16[q] = (uint16_t)(H.colind[k] - base[b]);
      else pcol[q] = H.colind[k];
    }
  }
  P.kind = sorted ? PadKind::sorted : idx16 ? PadKind::pad16 : PadKind::pad32;
  P.col32.swap(pcol);
  P.c16.swap(pc16);
  P.c8.swap(pc8);
  perm.swap(pperm);
  return P;
}

// ------------------------------------------------------------------------------------------------ row groups of k_spmv_rgcs

struct RgcsLayout {
  bool ok = false;
  std::vector<uint32_t> pidx;      // nstore words: (slot << kRgcsColBits) | (col - cmin)
  std::vector<int32_t> vperm;      // nstore: vals[t] = A.vals[vperm[t]], -1 in the padding
  std::vector<RgcsGroup> groups;
  std::vector<uint16_t> tptr;      // per tile R + 1 boundaries, and the two tail entries the kernel reads unconditionally
  int budget = 0;                  // nonzero budget of a group (the padded layout's stride)
  bool padded = false;
  int64_t nstore = 0;
  std::vector<int32_t> csr_pos;    // padded: where every CSR slot of A sits in the row-group array (pad_blocks builds A' on it)
  std::vector<Range2> col_range;   // per group its first and last column
};

// Row-group column-sorted copy of A (see k_spmv_rgcs).  Not built (ok = false) when a group spans >= 2^21 columns.
// compute_units: of the device; tiles_override > 0: tiles per group (tuning); phase_order = false: plain column order (A/B).
inline RgcsLayout build_rgcs(const HostCsr& H, int compute_units, int tiles_override, bool phase_order) {
  RgcsLayout D;
  const int64_t nnz = (int64_t)H.colind.size();
  if (nnz == 0) return D;
  std::vector<RgcsGroup>& groups = D.groups;
  std::vector<uint32_t> pidx(nnz);
  std::vector<int32_t> vperm(nnz);
  std::vector<uint16_t>& tptr = D.tptr;
  std::vector<int32_t> ord, lrow, cntr, nxt;
  // Nonzero budget of a group = a whole number of tiles (a workgroup pays the same latency for a partly filled
  // tile), chosen so that the groups fill the GPU's resident-workgroup slots (4 per CU at 32 KB of LDS) about once:
  // measured at the headline size, 1000 groups of 5 tiles run the product in ~30 us, 782 groups of 6.2 tiles in 37 us.
  int budget = kRgcsGroupNnz;
  {
    const int64_t slots = (int64_t)compute_units * 4;
    const double avg = (double)nnz / (double)std::max<int64_t>(H.nrows, 1);
    const int64_t kmax = std::max<int64_t>(1, (int64_t)(std::min<double>(kRgcsMaxRows * avg, kRgcsGroupNnz) / kRgcsTile));
    const int64_t k = std::min(kmax, std::max<int64_t>(1, (nnz + slots * kRgcsTile - 1) / (slots * kRgcsTile)));
    budget = (int)(k * kRgcsTile);
    if (tiles_override > 0) budget = (int)(std::min<int64_t>(kmax, tiles_override) * kRgcsTile);
  }
  auto group_end = [&](int64_t r) {
    int64_t r1 = r, nz = 0;
    while (r1 < H.nrows && r1 - r < kRgcsMaxRows) {
      const int64_t len = H.rowptr[r1 + 1] - H.rowptr[r1];
      if (nz + len > budget && r1 > r) break;
      nz += len;
      ++r1;
    }
    return r1;
  };
  // ORDER OF THE ENTRIES INSIDE A GROUP: by column PHASE, (col mod P), P = the typical width of a group's column window.
  // A workgroup sweeps its window tile by tile while all the groups of an XCD are resident together.  Sorted by column proper,
  // group g reads column c when its sweep gets there -- (c - cmin_g) / width of the way through the launch -- and the ~9
  // neighbouring groups whose windows overlap in c (PDE-like rows: the window moves by a fraction of its width from group to
  // group) read it at nine different times, spread over the whole launch, while the matrix streams through the same L2:
  // the x window was fetched 2.6 times (profiles/r03_pmc_traffic.json: 1.15 x the product's algorithmic bytes).  Sorted by
  // phase every group is at the same ABSOLUTE columns at the same time -- a rotation of its column order, any order is valid
  // -- and the overlap is served by the L2.  Windows as wide as the matrix (random patterns): P covers it, plain column order.
  int64_t P = INT64_MAX;
  {
    std::vector<int64_t> widths;
    for (int64_t r = 0; r < H.nrows;) {
      const int64_t r1 = group_end(r);
      int64_t cmin = INT64_MAX, cmax = -1;
      for (int64_t k = H.rowptr[r]; k < H.rowptr[r1]; ++k) {
        cmin = std::min<int64_t>(cmin, H.colind[k]);
        cmax = std::max<int64_t>(cmax, H.colind[k]);
      }
      if (cmax >= cmin) widths.push_back(cmax - cmin + 1);
      r = r1;
    }
    if (!widths.empty()) {
      std::nth_element(widths.begin(), widths.begin() + widths.size() / 2, widths.end());
      const int64_t med = std::max<int64_t>(1, widths[widths.size() / 2]);
      // the period: the WIDEST of the typical windows (those within 1.5 x the median), so that (col mod P) is one-to-one on
      // every typical group's window -- a pure rotation of its column order.  (The median itself -- rounds 3 -- left half of the
      // groups a little wider than the period: the first and last few columns of such a window share phases and their
      // entries INTERLEAVE in the sorted order, which cuts the contiguous per-group runs the shared-value layout of A'
      // builds on into slivers.)
      P = med;
      for (const int64_t w : widths)
        if (w <= med + med / 2) P = std::max(P, w);
    }
    if (!phase_order) P = INT64_MAX;
  }
  int64_t r = 0;
  while (r < H.nrows) {
    const int64_t r1 = group_end(r);
    const int R = (int)(r1 - r);
    const int e0 = H.rowptr[r], e1 = H.rowptr[r1], cnt = e1 - e0;
    int cmin = INT32_MAX, cmax = -1;
    for (int k = e0; k < e1; ++k) {
      cmin = std::min(cmin, H.colind[k]);
      cmax = std::max(cmax, H.colind[k]);
    }
    if (cnt == 0) cmin = cmax = 0;
    if ((int64_t)cmax - cmin >= (1ll << kRgcsColBits)) return RgcsLayout{};  // not representable: keep CSR-stream
    lrow.resize(cnt);
    for (int rr = 0; rr < R; ++rr)
      for (int k = H.rowptr[r + rr]; k < H.rowptr[r + rr + 1]; ++k) lrow[k - e0] = rr;
    ord.resize(cnt);
    for (int k = 0; k < cnt; ++k) ord[k] = k;
    // (a group much wider than the typical window would interleave several column ranges in one tile: plain order for it)
    // (P = INT64_MAX -- no period -- is plain order already; asked first: P + P / 2 would overflow)
    const int64_t Pg = P == INT64_MAX || (int64_t)cmax - cmin + 1 > P + P / 2 ? INT64_MAX : P;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
      const int64_t ca = H.colind[e0 + a], cb = H.colind[e0 + b];
      const int64_t pa = ca % Pg, pb = cb % Pg;
      return pa != pb ? pa < pb : ca < cb;
    });
    const int ntile = (cnt + kRgcsTile - 1) / kRgcsTile;
    const int32_t tp_start = (int32_t)tptr.size();
    for (int t = 0; t < ntile; ++t) {
      const int a = t * kRgcsTile, b = std::min(cnt, a + kRgcsTile);
      cntr.assign(R + 1, 0);
      for (int k = a; k < b; ++k) cntr[lrow[ord[k]] + 1]++;
      for (int rr = 0; rr < R; ++rr) cntr[rr + 1] += cntr[rr];
      for (int rr = 0; rr <= R; ++rr) tptr.push_back((uint16_t)cntr[rr]);
      nxt.assign(cntr.begin(), cntr.end() - 1);
      for (int k = a; k < b; ++k) {
        const int src = ord[k];
        const int slot = nxt[lrow[src]]++;
        pidx[e0 + k] = ((uint32_t)slot << kRgcsColBits) | (uint32_t)(H.colind[e0 + src] - cmin);
        vperm[e0 + k] = e0 + src;
      }
    }
    D.col_range.push_back(Range2{cmin, cmax});
    RgcsGroup gd{};
    gd.r0 = (int32_t)r;
    gd.R = R;
    gd.e0 = e0;
    gd.e1 = e1;
    gd.cmin = cmin;
    gd.tp = tp_start;
    groups.push_back(gd);
    if (ntile == 0)
      for (int rr = 0; rr <= R; ++rr) tptr.push_back(0);
    r = r1;
  }
  tptr.push_back(0);
  tptr.push_back(0);  // the kernel reads two uint16 at once
  // Padded layout (k_spmv_rgcs<.., PAD>): group g at [g * budget, ...), zero entries up to the end of its last tile.
  bool padded = (int64_t)groups.size() * budget < (int64_t)INT32_MAX;
  for (const RgcsGroup& gd : groups) padded = padded && gd.e1 - gd.e0 <= budget;
  int64_t nstore = nnz;
  if (padded) {
    nstore = (int64_t)groups.size() * budget;
    std::vector<uint32_t> pp((size_t)nstore, 0u);
    std::vector<int32_t> vp((size_t)nstore, -1);
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      RgcsGroup& gd = groups[gi];
      const int cnt = gd.e1 - gd.e0;
      const size_t dst = gi * (size_t)budget;
      for (int k = 0; k < cnt; ++k) {
        pp[dst + k] = pidx[gd.e0 + k];
        vp[dst + k] = vperm[gd.e0 + k];
      }
      const int full = (cnt + kRgcsTile - 1) / kRgcsTile * kRgcsTile;
      for (int k = cnt; k < full; ++k) pp[dst + k] = (uint32_t)(k % kRgcsTile) << kRgcsColBits;  // unused slot, value 0
    }
    pidx.swap(pp);
    vperm.swap(vp);
    D.csr_pos.assign((size_t)nnz, -1);
    for (int64_t p = 0; p < nstore; ++p)
      if (vperm[p] >= 0) D.csr_pos[vperm[p]] = (int32_t)p;
  }
  D.pidx.swap(pidx);
  D.vperm.swap(vperm);
  D.budget = budget;
  D.padded = padded;
  D.nstore = nstore;
  D.ok = true;
  return D;
}

// ------------------------------------------------------------------------------------------------ the one-launch iteration

// Per row group the range of A' blocks (boundaries rb, every one on a multiple of 8 rows) that own the 128-byte lines of the
// long pair -- 8 rows of n -- it gathers from.
inline std::vector<Range2> fused_dep(const std::vector<int32_t>& rb, const std::vector<Range2>& col_range, int64_t n) {
  const int nblk = (int)rb.size() - 1;
  std::vector<Range2> dep(col_range.size());
  for (size_t g = 0; g < col_range.size(); ++g) {
    const int64_t lo = col_range[g].x & ~7, hi = std::min<int64_t>((int64_t)col_range[g].y | 7, n - 1);
    const int b0 = (int)(std::upper_bound(rb.begin(), rb.end(), (int32_t)lo) - rb.begin()) - 1;
    const int b1 = (int)(std::upper_bound(rb.begin(), rb.end(), (int32_t)hi) - rb.begin()) - 1;
    dep[g] = Range2{std::max(b0, 0), std::min(std::max(b1, 0), nblk - 1)};
  }
  return dep;
}

// Several iterations per launch: per A' block the row groups whose rows of the short pair it gathers (the mirror image of
// `dep`; a cover by ONE range -- waiting for more is safe; a block nobody gathers from -- empty columns -- waits for every
// group: its own previous incarnation is then complete too).
inline std::vector<Range2> fused_bdep(const std::vector<Range2>& dep, int nblk) {
  const int ng = (int)dep.size(), nb = nblk;
  std::vector<Range2> bdep((size_t)nb, Range2{INT32_MAX, -1});
  for (int g = 0; g < ng; ++g)
    for (int L = dep[g].x; L <= dep[g].y; ++L) {
      bdep[L].x = std::min(bdep[L].x, g);
      bdep[L].y = std::max(bdep[L].y, g);
    }
  for (int L = 0; L < nb; ++L)
    if (bdep[L].y < bdep[L].x) bdep[L] = Range2{0, ng - 1};
  return bdep;
}

// The one-launch iteration of a halo-sharded solver: which A' blocks deposit the raw sums of the two overlap regions (rows
// [0, ovl) and [n - ovr, n)), and which row groups gather from a region: they wait for the halo_gf finish workgroups, whose
// flags follow the blocks'.
struct HaloDep {
  Range2 depL, depR;
  std::vector<Range2> dep2;
};
inline HaloDep fused_halo_dep(const std::vector<int32_t>& rb, const std::vector<Range2>& col_range, int64_t n, int64_t ovl,
                              int64_t ovr, int halo_gf) {
  const int nblk = (int)rb.size() - 1;
  HaloDep D;
  auto block_of = [&](int64_t row) { return (int)(std::upper_bound(rb.begin(), rb.end(), (int32_t)row) - rb.begin()) - 1; };
  D.depL = ovl > 0 ? Range2{0, std::max(block_of(ovl - 1), 0)} : Range2{1, 0};
  D.depR = ovr > 0 ? Range2{std::max(block_of(n - ovr), 0), nblk - 1} : Range2{1, 0};
  D.dep2.resize(col_range.size());
  for (size_t g = 0; g < D.dep2.size(); ++g) {
    const int64_t lo = col_range[g].x & ~7, hi = std::min<int64_t>((int64_t)col_range[g].y | 7, n - 1);
    const bool touches = lo < ovl || hi >= n - ovr;
    D.dep2[g] = touches ? Range2{nblk, nblk + halo_gf - 1} : Range2{1, 0};
  }
  return D;
}

}  // namespace fpsq
