// fpsq_structure.hip.h -- fpsq_set_structure's device side: uploads of the layouts fpsq_layout.h builds, the workspaces, the
// set-up of the one-launch iteration (setup_fused_iteration, setup_fused_halo), finish_structure.
// Part of fpsq.hip's translation unit.
#pragma once

#include "fpsq_handle.hip.h"
#include "fpsq_layout.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

// ------------------------------------------------------------------ host-side sparse set-up
// Every stored layout is BUILT by fpsq_layout.h (plain host code, checked on the CPU by tests/host/layout_check.cpp); what
// follows uploads what the builders return, one function per layout.

static_assert(sizeof(BlkDesc) == sizeof(int4) && sizeof(SegDesc) == sizeof(uint4) && sizeof(Range2) == sizeof(int2),
              "fpsq_layout.h: host images of the descriptor arrays the kernels read as int4 / uint4 / int2");
static_assert(sizeof(RgcsGroup) == 32, "two 16-byte loads at the head of a row group's workgroup");

template <class T>
int upload(fpsq_handle h, T* dst, const std::vector<T>& src) {
  if (!src.empty()) HIPCHK(h, hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
template <class T>
int dalloc_upload(fpsq_handle h, T** p, const std::vector<T>& src) {
  if (int rc = dalloc(h, p, src.size())) return rc;
  return upload(h, *p, src);
}

int upload_blocks(fpsq_handle h, const HostCsr& H, const BlockLayout& B, DevCsr& D) {
  D.nrows = H.nrows;
  D.ncols = H.ncols;
  D.nnz = (int64_t)H.colind.size();
  D.nstore = D.nnz;
  D.nblk = B.nblk();
  if (int rc = dalloc(h, &D.rowptr, H.rowptr.size())) return rc;
  // one padding entry (column 0, value 0): the product kernels read index `s` of an empty row block unconditionally
  if (int rc = dalloc(h, &D.colind, H.colind.size() + 1)) return rc;
  if (int rc = dalloc(h, &D.vals, H.colind.size() + 1)) return rc;
  HIPCHK(h, hipMemset(D.colind + H.colind.size(), 0, 4));
  HIPCHK(h, hipMemset(D.vals + H.colind.size(), 0, 8));
  if (int rc = dalloc(h, &D.rowblk, B.rb.size())) return rc;
  if (int rc = upload(h, D.rowptr, H.rowptr)) return rc;
  if (int rc = upload(h, D.colind, H.colind)) return rc;
  if (int rc = upload(h, D.rowblk, B.rb)) return rc;
  if (int rc = dalloc(h, &D.blkdesc, B.blkdesc.size())) return rc;
  HIPCHK(h, hipMemcpy(D.blkdesc, B.blkdesc.data(), B.blkdesc.size() * sizeof(int4), hipMemcpyHostToDevice));
  if (B.has_col16) {
    if (int rc = dalloc_upload(h, &D.col16, B.col16)) return rc;
    if (int rc = dalloc_upload(h, &D.colbase, B.colbase)) return rc;
    D.win = B.win;
  }
  return 0;
}

// Re-store uploaded blocks in the padded layout pad_blocks() built (k_spmv<.., PAD>; nothing to do when it declined).
// ext_vals / zero_pos (shared values): the row-group array of A the blocks read, and its entry that always holds 0.0.
int upload_padded(fpsq_handle h, const PaddedLayout& P, DevCsr& D, const double* ext_vals, int64_t zero_pos) {
  if (P.kind == PadKind::none) return 0;
  const bool shared = P.kind == PadKind::shared;
  // shared: what a refresh still has to fill is the side array of the blocks that keep their own values (+ 1: its padding)
  const size_t nvals = shared ? (size_t)P.nown * kSpmvNnz + 1 : P.slots;
  dfree(h, &D.vals);
  dfree(h, &D.col16);
  dfree(h, &D.colind);
  if (int rc = dalloc(h, &D.vals, nvals)) return rc;
  HIPCHK(h, hipMemset(D.vals, 0, nvals * 8));
  if (P.kind == PadKind::pad32) {
    if (int rc = dalloc_upload(h, &D.colind, P.col32)) return rc;
  } else if (P.kind == PadKind::pad16) {  // the 16-bit form is the only one the padded kernel reads
    if (int rc = dalloc_upload(h, &D.col16, P.c16)) return rc;
  } else {
    if (int rc = dalloc_upload(h, &D.cs16, P.c16)) return rc;
    if (int rc = dalloc_upload(h, &D.cs8, P.c8)) return rc;
    D.sorted = true;
  }
  if (shared) {
    if (int rc = dalloc(h, &D.segdesc, P.segdesc.size())) return rc;
    HIPCHK(h, hipMemcpy(D.segdesc, P.segdesc.data(), P.segdesc.size() * sizeof(uint4), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(D.blkdesc, P.blkdesc.data(), P.blkdesc.size() * sizeof(int4), hipMemcpyHostToDevice));
    D.shared = true;
    D.vals_ext = ext_vals;
    D.zero_pos = zero_pos;
  }
  D.padded = true;
  D.nstore = shared ? (int64_t)P.nown * kSpmvNnz : (int64_t)P.slots;
  return 0;
}

// Row-group column-sorted copy of A (k_spmv_rgcs): one padding entry behind the index words and the values
int upload_rgcs(fpsq_handle h, const HostCsr& H, const RgcsLayout& L, DevRgcs& D) {
  D.ok = false;
  if (!L.ok) return 0;
  uint32_t* dp;
  RgcsGroup* dg;
  uint16_t* d5;
  if (int rc = dalloc(h, &dp, (size_t)L.nstore + 1)) return rc;
  if (int rc = dalloc(h, &D.vals, (size_t)L.nstore + 1)) return rc;
  if (int rc = dalloc(h, &D.vperm, (size_t)L.nstore)) return rc;
  if (int rc = dalloc(h, &dg, L.groups.size())) return rc;
  if (int rc = dalloc(h, &d5, L.tptr.size() + 2)) return rc;
  if (int rc = upload(h, dp, L.pidx)) return rc;
  HIPCHK(h, hipMemset(dp + L.nstore, 0, 4));
  HIPCHK(h, hipMemset(D.vals, 0, ((size_t)L.nstore + 1) * 8));
  if (int rc = upload(h, D.vperm, L.vperm)) return rc;
  if (int rc = upload(h, dg, L.groups)) return rc;
  if (int rc = upload(h, d5, L.tptr)) return rc;
  D.view = RgcsView{dp, D.vals, dg, d5, (int32_t)L.groups.size(), (int32_t)H.nrows, L.padded ? L.budget : 0};
  D.nstore = L.nstore;
  D.nnz = (int64_t)H.colind.size();
  D.ok = true;
  return 0;
}

inline int npart_A(fpsq_handle h) { return h->RA.ok ? h->RA.view.ng : h->A.nblk; }
// Sums over the ranks need no launch of their own: one GPU; a communicator of ONE rank (nobody to add to); or the halo-sharded
// layout on a peer-to-peer route whose ranks form them inside the launches that need them (Comm::xch_table, known after arm()).
inline bool insum(fpsq_handle h) {
  return !h->comm || (h->halo && (h->comm->nranks == 1 || h->comm->xch_table() != nullptr));
}
// ... and when other ranks exist: the table the kernels are given (null: one GPU, or a communicator of one)
inline const XchTable* insum_table(fpsq_handle h) { return h->comm && h->comm->nranks > 1 ? h->comm->xch_table() : nullptr; }
inline int64_t n_owned(fpsq_handle h) { return h->halo ? h->n - h->ovr : h->n; }
// the number of the next in-launch sum over the ranks (0 means "no exchange" to the kernels: skipped when the counter wraps)
inline uint32_t next_xseq(fpsq_handle h) {
  if (++h->xch_seq == 0) ++h->xch_seq;
  return h->xch_seq;
}

int alloc_workspaces(fpsq_handle h) {
  const size_t n = (size_t)h->n, m = (size_t)h->m;
  if (int rc = dalloc(h, &h->LP, 2 * n)) return rc;
  if (int rc = dalloc(h, &h->SP, 2 * m)) return rc;
  if (int rc = dalloc(h, &h->SP2, 2 * m)) return rc;
  if (int rc = dalloc(h, &h->comm_vec, 2 * n)) return rc;
  double** nv[] = {&h->Cx, &h->Cw2, &h->in_n1, &h->in_n2, &h->p1, &h->p2b,
                   &h->gs, &h->gx, &h->jc, &h->g, &h->xin, &h->xk};
  for (auto p : nv)
    if (int rc = dalloc(h, p, n)) return rc;
  double** mv[] = {&h->Lw[0], &h->Lw[1], &h->Lx[0], &h->Lx[1], &h->Cw, &h->Cy, &h->in_m, &h->ys, &h->c,
                   &h->Mr[0], &h->Mr[1], &h->Mw[0], &h->Mw[1], &h->Mx};
  for (auto p : mv)
    if (int rc = dalloc(h, p, m)) return rc;
  h->npS = std::max(std::max(std::max(h->A.nblk, h->AT.nblk), kEwBlocksMax), npart_A(h));
  if (int rc = dalloc(h, &h->pS, (size_t)h->npS * 2)) return rc;
  if (int rc = dalloc(h, &h->pS2, (size_t)h->npS * 2)) return rc;
  if (int rc = dalloc(h, &h->pS2b, (size_t)h->npS * 2)) return rc;
  h->strT = h->AT.nblk;
  h->strA = npart_A(h);
  double** ev[] = {&h->pW[0], &h->pW[1], &h->pWalt[0], &h->pWalt[1], &h->pE, &h->pE2, &h->pE3, &h->pQ[0], &h->pQ[1], &h->pC[0], &h->pC[1],
                   &h->pEm[0], &h->pEm[1]};
  for (auto p : ev)
    if (int rc = dalloc(h, p, (size_t)kEwBlocksMax * 2)) return rc;
  if (!h->mm_ptag) {
    if (int rc = dalloc(h, &h->mm_ptag, (size_t)kEwBlocksMax * 2)) return rc;
    HIPCHK(h, hipMemset(h->mm_ptag, 0, (size_t)kEwBlocksMax * 16));
  }
  return 0;
}

// One launch per joint iteration (k_iter_fused) -- what it needs beyond the two products' layouts: every A' block boundary on a
// 128-byte line of the long pair, the main layouts of both products (column-sorted padded blocks, padded row groups), 32-bit
// byte offsets into the long pair, and per row group the range of A' blocks that own the lines it gathers from (fused_dep).
// rb: the row blocks of A'.
int setup_fused_iteration(fpsq_handle h, const std::vector<int32_t>& rb, const std::vector<Range2>& col_range) {
  h->fuse_ok = false;
  if (!h->fuse_iter || !h->fuse_hw_ok || !h->RA.ok || h->RA.view.stride == 0 || !h->AT.padded || !(h->AT.sorted || h->AT.col16) || h->AT.nblk < 1)
    return 0;
  if ((int64_t)h->n * 16 >= (int64_t)INT32_MAX || (int64_t)h->m * 16 >= (int64_t)INT32_MAX) return 0;
  if ((int)col_range.size() != h->RA.view.ng) return 0;
  if ((int)rb.size() - 1 != h->AT.nblk || !rowblocks_aligned(rb, 8)) return 0;
  const std::vector<Range2> dep = fused_dep(rb, col_range, h->n);
  if (h->fuse_iter == 1) {
    // Where it pays (measured): a grid of several resident sets -- the row groups then enter as the last A'
    // blocks drain and find most of what they wait for done -- whose row groups depend on a small part of the A' blocks.
    // A grid that is resident at once gains nothing from sharing a launch and pays for the flags (cfg2, random columns: every
    // group waits for every block; 2500 -> 2230 evals/s).
    double width = 0.0;
    for (const Range2& d : dep) width += d.y - d.x + 1;
    width /= (double)std::max<size_t>(dep.size(), 1);
    // (the size threshold: profiles/r04_fused_sizes.txt -- headline generator, one launch against two: -3.2 % at 1225 blocks,
    // -2.4 % at 1617, +2.3 % at 1764, +7.7 % at 1862, +8.4 % at 1960, +7.3 % at 2450, +2.5 to +4 % at 4900, -0.5 % at 9800)
    if (h->AT.nblk < 17 * h->resident_wgs / 10 || width > h->AT.nblk / 8.0) return 0;
  }
  dfree(h, &h->fz_dep);
  dfree(h, &h->fz_flag);
  dfree(h, &h->fz_ptag);
  if (int rc = dalloc(h, &h->fz_dep, dep.size())) return rc;
  // (+ kEwBlocksMax entries: the finish workgroups of a halo-sharded handle publish themselves behind the blocks)
  if (int rc = dalloc(h, &h->fz_flag, (size_t)h->AT.nblk + kEwBlocksMax)) return rc;
  if (int rc = dalloc(h, &h->fz_ptag, ((size_t)h->AT.nblk + kEwBlocksMax) * 4)) return rc;
  HIPCHK(h, hipMemcpy(h->fz_dep, dep.data(), dep.size() * sizeof(int2), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemset(h->fz_flag, 0, ((size_t)h->AT.nblk + kEwBlocksMax) * 4));
  HIPCHK(h, hipMemset(h->fz_ptag, 0, ((size_t)h->AT.nblk + kEwBlocksMax) * 32));
  h->fz_rb = rb;
  h->fz_colrange = col_range;
  h->fuse_ok = true;
  // ---- several iterations per launch (fpsq_multi.hip.h): per A' block the row groups whose rows of the short pair it gathers
  // (fused_bdep), second copies of the flags and tagged words, records, the second long pair
  h->multi_ok = false;
  if (h->multi_max > 1) {
    const int ng = h->RA.view.ng, nb = h->AT.nblk;
    const std::vector<Range2> bdep = fused_bdep(dep, nb);
    dfree(h, &h->mz_bdep);
    dfree(h, &h->mz_flag2);
    dfree(h, &h->mz_ptag2);
    if (int rc = dalloc(h, &h->mz_bdep, bdep.size())) return rc;
    HIPCHK(h, hipMemcpy(h->mz_bdep, bdep.data(), bdep.size() * sizeof(int2), hipMemcpyHostToDevice));
    if (int rc = dalloc(h, &h->mz_flag2, (size_t)nb + kEwBlocksMax)) return rc;
    if (int rc = dalloc(h, &h->mz_ptag2, ((size_t)nb + kEwBlocksMax) * 4)) return rc;
    HIPCHK(h, hipMemset(h->mz_flag2, 0, ((size_t)nb + kEwBlocksMax) * 4));
    HIPCHK(h, hipMemset(h->mz_ptag2, 0, ((size_t)nb + kEwBlocksMax) * 32));
    for (int q = 0; q < 2; ++q) {
      dfree(h, &h->mz_gflag[q]);
      dfree(h, &h->mz_atag[q]);
      if (int rc = dalloc(h, &h->mz_gflag[q], (size_t)ng)) return rc;
      if (int rc = dalloc(h, &h->mz_atag[q], (size_t)ng * 4)) return rc;
      HIPCHK(h, hipMemset(h->mz_gflag[q], 0, (size_t)ng * 4));
      HIPCHK(h, hipMemset(h->mz_atag[q], 0, (size_t)ng * 32));
      if (!h->mz_utag[q]) {
        if (int rc = dalloc(h, &h->mz_utag[q], (size_t)4 * kEwBlocksMax * 2)) return rc;
        HIPCHK(h, hipMemset(h->mz_utag[q], 0, (size_t)4 * kEwBlocksMax * 16));
      }
    }
    if (!h->mz_rec_h) {
      const size_t words = (size_t)2 * kRecRing * 512 + (size_t)kRecRing * 2 * kSrecSlot + 8;
      if (int rc = dalloc(h, &h->mz_rec_h, words)) return rc;
      HIPCHK(h, hipMemset(h->mz_rec_h, 0, words * 8));
      h->mz_rec_m = h->mz_rec_h + (size_t)kRecRing * 512;
      h->mz_srec = h->mz_rec_m + (size_t)kRecRing * 512;
      h->mz_hdone = h->mz_srec + (size_t)kRecRing * 2 * kSrecSlot;
    }
    if (!h->LP2)
      if (int rc = dalloc(h, &h->LP2, 2 * (size_t)h->n)) return rc;
    h->multi_ok = true;
  }
  return 0;
}

// The one-launch iteration of a halo-sharded handle (fpsq_comm_set_halo, or a new structure on such a handle): which A' blocks
// deposit the raw sums of the two overlap regions, and which row groups gather from a region (they wait for the finish
// workgroups) -- fused_halo_dep.  Needs the regions on 128-byte lines of the long pair (8 rows): distributed.halo_plan rounds
// its windows so.
int setup_fused_halo(fpsq_handle h) {
  h->fuse_halo_ok = false;
  if (!h->fuse_ok || !h->halo || h->ovl + h->ovr == 0) return 0;
  if (h->ovl % 8 != 0 || (h->n - h->ovr) % 8 != 0 || h->halo_gf > kEwBlocksMax) return 0;
  const HaloDep hd = fused_halo_dep(h->fz_rb, h->fz_colrange, h->n, h->ovl, h->ovr, h->halo_gf);
  h->fz_depL = make_int2(hd.depL.x, hd.depL.y);
  h->fz_depR = make_int2(hd.depR.x, hd.depR.y);
  dfree(h, &h->fz_dep2);
  if (int rc = dalloc(h, &h->fz_dep2, hd.dep2.size())) return rc;
  HIPCHK(h, hipMemcpy(h->fz_dep2, hd.dep2.data(), hd.dep2.size() * sizeof(int2), hipMemcpyHostToDevice));
  h->fuse_halo_ok = true;
  return 0;
}

// after the structure (host CSR of A) is known: transposed copy, the layouts (built on the host from the switches read here,
// then uploaded), workspaces
int finish_structure(fpsq_handle h, const HostCsr& HA) {
  HostCsr HT;
  std::vector<int32_t> perm;
  transpose_structure(HA, HT, perm);
  const bool compact = h->opt.jac_format == 1;  // plain CSR with 32-bit columns: no compressed, padded or row-group layout
  h->AT.row_align = h->fuse_iter ? 8 : 1;  // (whether a sharded handle may use the launch is decided per run: KrylovRun::setup)
  if (const char* ev = std::getenv("FPSQ_AT_ROW_ALIGN")) h->AT.row_align = std::max(1, std::atoi(ev));  // (tests: the fused layout without the fused launch)
  if (int rc = upload_blocks(h, HA, build_blocks(HA, h->A.row_align, !compact), h->A)) return rc;
  BlockLayout BT = build_blocks(HT, h->AT.row_align, !compact);  // (the row blocks of A': computed once, for all that follows)
  if (int rc = upload_blocks(h, HT, BT, h->AT)) return rc;
  // (once uploaded, the large host arrays nobody reads again go before the next builder allocates its own)
  std::vector<uint16_t>().swap(BT.col16);
  RgcsLayout LA;
  if (!compact) {
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, h->opt.device) == hipSuccess && prop.multiProcessorCount > 0)
      cus = prop.multiProcessorCount;
    const char* tiles = std::getenv("FPSQ_RGCS_TILES");  // tuning override: tiles per group
    const char* phase = std::getenv("FPSQ_RGCS_PHASE");  // 0: plain column order (A/B)
    LA = build_rgcs(HA, cus, tiles ? std::max(1, std::atoi(tiles)) : 0, !(phase && std::atoi(phase) == 0));
  }
  if (int rc = upload_rgcs(h, HA, LA, h->RA)) return rc;
  std::vector<uint32_t>().swap(LA.pidx);
  std::vector<int32_t>().swap(LA.vperm);
  if (!compact) {
    const bool can_share = h->RA.ok && !LA.csr_pos.empty() && !h->refresh_3pass;
    const PaddedLayout PT = pad_blocks(HT, BT, perm, h->at_sorted, h->at_shared, can_share ? &LA.csr_pos : nullptr, h->RA.nstore);
    if (PT.nown >= 0 && std::getenv("FPSQ_VERBOSE"))
      std::fprintf(stderr, "fpsq: shared A' values: %d of %d blocks keep their own\n", PT.nown, BT.nblk());
    if (int rc = upload_padded(h, PT, h->AT, h->RA.vals, h->RA.nstore)) return rc;
  }
  if (int rc = dalloc_upload(h, &h->permT, perm)) return rc;
  h->nnz = h->A.nnz;
  // COO input without duplicates: the value permutations of A' and of the row groups are composed with the COO -> CSR order
  // once, here, so that a refresh gathers straight from the caller's jac_coord! output (k_refresh) -- no CSR staging pass.
  // (With duplicates the slots are summed into the CSR array first and the permutations keep pointing there.)
  h->perms_to_input = false;
  if (h->in_perm && !h->in_slotptr && !h->refresh_3pass && h->nnz > 0) {
    if (h->AT.nstore > 0)
      hipLaunchKernelGGL(k_compose_perm, dim3(ew_grid(h->AT.nstore)), dim3(kBlock), 0, nullptr, h->permT, h->in_perm, h->AT.nstore);
    if (h->RA.ok)
      hipLaunchKernelGGL(k_compose_perm, dim3(ew_grid(h->RA.nstore)), dim3(kBlock), 0, nullptr, h->RA.vperm, h->in_perm, h->RA.nstore);
    h->perms_to_input = true;
  }
  if (int rc = alloc_workspaces(h)) return rc;
  if (int rc = setup_fused_iteration(h, BT.rb, LA.col_range)) return rc;
  if (int rc = setup_fused_halo(h)) return rc;  // (a halo-sharded handle given a new structure)
  HIPCHK(h, hipDeviceSynchronize());  // the set-up used null-stream copies/memsets; the solver stream is non-blocking
  h->have_structure = true;
  h->have_values = false;
  h->info.n = h->n;
  h->info.m = h->m;
  h->info.nnz = h->nnz;
  h->info.spmv_a_blocks = npart_A(h);
  h->info.spmv_at_blocks = h->AT.nblk;
  h->info.at_sorted = h->AT.shared ? 2 : h->AT.sorted ? 1 : 0;
  return 0;
}

}  // namespace
