// fpsq_handle.hip.h -- the handle: the device images of the stored layouts (DevCsr, DevRgcs), fpsq_solver_s and fpsq_qp_s,
// and what every function that holds a handle uses (HIPCHK, dalloc / xalloc / dfree, ew_grid).
// Part of fpsq.hip's translation unit.
#pragma once

#include "../../include/fpsq.h"
#include "fpsq_spmv.hip.h"
#include "fpsq_multi.hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace fpsq;

namespace {

struct DevCsr {
  int64_t nrows = 0, ncols = 0, nnz = 0;
  int32_t* rowptr = nullptr;
  int32_t* colind = nullptr;
  double* vals = nullptr;
  int32_t* rowblk = nullptr;
  int32_t nblk = 0;
  int32_t row_align = 1;       // make_rowblocks' alignment of the block boundaries (8 for the A' of a fused-iteration handle)
  uint16_t* col16 = nullptr;   // compressed columns (see CsrView), null when not representable
  int32_t* colbase = nullptr;
  int4* blkdesc = nullptr;
  bool padded = false;         // vals / col16 / colind hold nblk blocks of kSpmvNnz slots (see k_spmv<.., PAD>)
  int64_t nstore = 0;          // stored value slots: nnz, or nblk * kSpmvNnz when padded
  int32_t win = 0;             // with col16: widest column span of a row block
  uint16_t* cs16 = nullptr;    // column-sorted padded blocks (k_spmv<.., CSORT>): slot | (col & 31) << 11 ...
  uint8_t* cs8 = nullptr;      // ... and col >> 5 of every stored entry; col16 is then not kept
  bool sorted = false;
  // SHARED VALUES (A' only; see pad_blocks): the blocks hold no values of their own -- every entry is read from the row-group
  // copy of A (`vals_ext` = DevRgcs::vals), located through one 16-byte descriptor per 64 consecutive entries
  uint4* segdesc = nullptr;
  const double* vals_ext = nullptr;
  int64_t zero_pos = 0;
  bool shared = false;
  CsrView view() const {
    return CsrView{rowptr, colind, shared ? vals_ext : vals, rowblk, nblk, (int32_t)nrows, col16, colbase, blkdesc, cs16, cs8, segdesc,
                   (int32_t)zero_pos, vals};
  }
};

struct EventPair {
  hipEvent_t a, b;
};

struct DevRgcs {
  bool ok = false;
  RgcsView view{};
  double* vals = nullptr;
  int32_t* vperm = nullptr;  // vals[t] = A.vals[vperm[t]]
  int64_t nnz = 0;
  int64_t nstore = 0;        // stored value slots (> nnz in the padded layout)
};

}  // namespace

#include "fpsq_comm.hip.h"

struct fpsq_solver_s {
  int64_t n = 0, m = 0, nnz = 0;
  fpsq_options opt{};
  double delta = 0.0;
  hipStream_t stream = nullptr;
  bool in_stream_on = false;     // fpsq_set_input_stream: producer stream of device-resident arguments
  hipStream_t in_stream = nullptr;
  // One GPU, a registered producer stream (FPSQ_ADOPT_STREAM=0 switches it off): the library enqueues ON that stream instead of on one of its own -- inputs and outputs
  // are then ordered by the stream itself: no event record / wait pair at either end of a call, and no hops between two queues from
  // the last kernel of an evaluation to the first of the next (the caller's stream waits for the tail, the library's for the caller's)
  bool adopt_streams = true, adopted = false;
  hipStream_t own_stream = nullptr;
  hipEvent_t ev_in = nullptr;
  bool have_structure = false, have_values = false;
  std::string err;

  DevCsr A, AT;
  DevRgcs RA;                   // column-sorted row-group copy of A used by the A product when eligible
  int32_t* permT = nullptr;     // AT.vals[t] = A.vals[permT[t]]
  int64_t nnz_in = 0;           // length of the caller's value array (COO entries or CSR nnz)
  bool perms_to_input = false;  // COO structure without duplicates: permT / RA.vperm are composed down to the caller's array
  bool refresh_3pass = false;   // FPSQ_JAC_REFRESH=3: the three grid-stride gathers of rounds 1-3 (A/B, test)
  int32_t* in_perm = nullptr;   // COO path: sorted position -> caller index
  int32_t* in_slotptr = nullptr;// COO path with duplicates: CSR slot -> range of sorted positions
  double* in_vals = nullptr;    // staging of the caller's values (COO path)

  std::vector<void*> allocs;
  // Golub-Kahan vectors, [len][2] interleaved: LP = "long" (n) pair, SP = "short" (m) pair
  double *LP, *SP;
  double* SP2;                  // alternate short pair: the A product ping-pongs SP so fused updates may read the old one
  // n-vectors
  double *Cx, *Cw2, *in_n1, *in_n2, *p1, *p2b, *gs, *gx, *jc, *g, *xin, *xk;
  // m-vectors
  double *Lw[2], *Lx[2], *Cw, *Cy, *in_m, *ys, *c, *Mr[2], *Mw[2], *Mx;
  // partial-sum buffers
  double *pS, *pS2, *pW[2], *pE, *pE2, *pE3, *pQ[2], *pC[2];
  double* pS2b = nullptr;  // second array for the A product's partials: fused launches alternate (KrylovRun::pa_last)
  // second halves of the update partials.  A riding step and a riding update of ONE launch must never share an array:
  // the leaders of the step (sixteen workgroups, any of which another kernel may hold up) read, the update workgroups --
  // released by the record of their own XCC's leader -- write.  LSQR's / CRAIG's update partials therefore alternate
  // between pW[l] and pWalt[l] by iteration (run_krylov: upd_part), MINRES' stage E3 writes pWalt where E2 writes pW.
  double* pWalt[2];
  double* pEm[2];               // squared-norm partials of the m-vector right-hand sides (pE / pE2: of the n-vector ones)
  int npS = 0;
  int strT = 0, strA = 0;       // lane strides of pS (A' product partials) and pS2 (A product partials)
  LsqrState* lsqr[2];
  CraigState* craig;
  LsqrState* lsqr_alt[2];       // second copies: the target of a step that rides in a product launch (see run_krylov)
  CraigState* craig_alt;
  bool at_sorted = true;        // A' blocks stored column-sorted where representable (FPSQ_AT_SORTED=0: row order)
  bool at_shared = true;        // ... and without values of their own where the row groups of A can serve them (FPSQ_AT_SHARED=0)
  // steps riding with LEADERS (large grids, see fpsq_spmv.hip.h): the leaders' record (one line of device memory), a launch counter
  unsigned long long* ride_rec = nullptr;
  unsigned long long ride_seq = 0;
  bool ride_lead = true;        // FPSQ_RIDE_LEAD=0: large grids keep the stand-alone k_step
  bool ride_break = false;      // FPSQ_DEBUG_RIDE_BREAK=1 (tests): the leaders publish a wrong launch number, every wait expires
  int ride_delay = 0;           // FPSQ_DEBUG_RIDE_DELAY=c+1 (tests): leader c of every launch starts ~100 us late
  int resident_wgs = 1024;      // product workgroups (32 KB of LDS) the device holds at once: 4 per CU, measured
  bool atl_two = true;          // k_spmv_atl: two row blocks for the first resident set (FPSQ_ATL_TWO=0: one each)
  // one launch per joint iteration (k_iter_fused; FPSQ_FUSE_ITER=0: two launches)
  int ride_delay_mid = 0;       // FPSQ_DEBUG_RIDE_DELAY_MID=c+1 (tests): mid leader c of every fused launch starts ~100 us late
  int fuse_rotate = 0;          // FPSQ_DEBUG_FUSE_ROTATE=r (tests): the A' blocks of eighth e are written on XCD (e - r) & 7, gathered on XCD e
  bool minres_merge = true;     // MINRES lane: stage E1, step A and stage E2 as one launch (k_minres_mid; FPSQ_MINRES_MERGE=0: three)
  unsigned long long* mm_ptag = nullptr;  // its tagged partials (two words per element-wise workgroup)
  bool fuse_fell_back = false;  // an expired wait of a fused launch has just switched the handle to two launches per iteration
  bool fuse_break = false;      // FPSQ_DEBUG_FUSE_BREAK=1 (tests): the A' blocks of a fused launch publish a wrong number, every wait for them expires
  int fuse_iter = 1;            // 0: never; 1: where it pays (setup_fused_iteration); 2: wherever it is possible (tests)
  bool fuse_ok = false;
  // The in-launch hand-overs (riding leaders' records per XCC, written-through rows, blocks dealt to XCDs by blockIdx & 7) were
  // validated on gfx942 / gfx950 in SPX mode with 8 XCCs (tools/coherence_probe.hip): anything else keeps two launches per
  // iteration from the start instead of finding out through expired waits (advisor, round 4)
  bool fuse_hw_ok = false;
  bool verbose = false;         // FPSQ_VERBOSE=1: one line on stderr when a call is repeated on two launches per iteration
  int64_t mmid_launches = 0;    // k_minres_mid launches of the current call
  int mmid_cap = 0;             // workgroups of k_minres_mid the device holds at once (occupancy x CUs): its grid must fit with a margin
  int64_t loop_launches = 0, loop_iters = 0;  // the Krylov loop(s) of the current call (fpsq_info.last_loop_*)
  int2* fz_dep = nullptr;                 // per row group: the A' blocks it waits for
  // halo-sharded handles (setup_fused_halo, at fpsq_comm_set_halo): the finish workgroups a row group waits for, the A' blocks
  // that deposit the raw sums of the two overlap regions; what the set-up needs again then (block boundaries, column ranges)
  int2* fz_dep2 = nullptr;
  int2 fz_depL{1, 0}, fz_depR{1, 0};
  // several iterations per launch (k_iter_multi, fpsq_multi.hip.h; FPSQ_MULTI_ITER=k: at most k per launch, 1: off)
  // Default 1 = off.  Measured at the headline size (profiles/r05_multi_iter.txt): bitwise the one-launch iterations, 9 launches per
  // evaluation instead of 21, and NO gain -- 0.99-1.00 x: the kernel boundary it removes (2.6 us per iteration) is paid back inside the
  // launch (agent-scope gathers of the short pair, the second long pair, tagged publications: +2.8 us per iteration)
  int multi_max = 1;
  // real workgroups of the LSQR / CRAIG updates in a multi launch (FPSQ_MULTI_UPD=t,a; multiples of 8).  Default: one per
  // segment workgroup.  Fewer, each walking several -- so that the next iteration's A' blocks are dispatched sooner -- was measured
  // SLOWER at the headline size (64 / 192: 854 evals/s, 128 / 384: 926, all: 940 against 952 with one iteration per launch: the long
  // update then cannot keep up and the next mid leaders wait for it)
  int multi_upd_t = 1 << 20, multi_upd_a = 1 << 20;
  // FPSQ_MULTI_DEFER_LONG=1: CRAIG's long update one iteration later, behind the NEXT iteration's A' blocks, so that only the small
  // m-vector updates stand between an iteration's row groups and the next A' blocks in the dispatch order.  Measured SLOWER (909
  // against 949 evals/s at 8 iterations per launch: the long update then competes with the A' phase and holds the mid leaders up)
  bool multi_defer_long = false;
  bool multi_ok = false;
  int2* mz_bdep = nullptr;
  unsigned int* mz_flag2 = nullptr;          // second parity of fz_flag / fz_ptag
  unsigned long long* mz_ptag2 = nullptr;
  unsigned int* mz_gflag[2] = {nullptr, nullptr};
  unsigned long long* mz_atag[2] = {nullptr, nullptr};
  unsigned long long* mz_utag[2] = {nullptr, nullptr};
  unsigned long long *mz_rec_h = nullptr, *mz_rec_m = nullptr, *mz_srec = nullptr, *mz_hdone = nullptr;
  double* LP2 = nullptr;                      // the second long pair
  int64_t multi_launches = 0, multi_iters = 0;
  bool fuse_halo_ok = false;
  bool fuse_halo_on = true;               // FPSQ_FUSE_HALO=0: a handle with shared rows keeps the halo launch between two product launches
  std::vector<int32_t> fz_rb;
  std::vector<Range2> fz_colrange;
  unsigned int* fz_flag = nullptr;        // per A' block: launch number of its last completion
  unsigned long long* fz_ptag = nullptr;  // per A' block: four tagged words (its squared-norm partials)
  unsigned long long* ride_rec2 = nullptr;  // the mid leaders' record
  void* state3[3] = {nullptr, nullptr, nullptr};  // third copies of the LSQR (x 2) / CRAIG / LNLQ states: lsqr, craig, lnlq
  int64_t fused_launches = 0, fused_total = 0;
  // developer probe (FPSQ_FUSE_PROBE=<file>, FPSQ_FUSE_PROBE_AT=<n-th fused launch of the handle>): per-workgroup time stamps of one launch
  int64_t fuse_probe_at = 0;
  bool fuse_tail = true;               // FPSQ_FUSE_TAIL=0: the raw A'[q1, c] product and k_qp_penalty_grad as two launches (one GPU; bitwise the same)
  unsigned long long* fuse_probe_buf = nullptr;
  int fuse_probe_grid = 0;
  std::vector<int> fuse_probe_layout;
  std::string fuse_probe_path;
  bool at_xcd = true;           // k_spmv_atl: every XCD walks a contiguous eighth of the row blocks (FPSQ_AT_XCD=0: grid order)
  MinresState* minres;
  LnlqState* lnlq;
  LnlqState* lnlq_alt;          // (second copy, see lsqr_alt)
  MinresState* minres_alt;
  LaneCtl* ctl_tmp;
  LaneCtl* ctl_raw;             // constant {ca = 1, cb = 0, done = 0}: raw partial products before an all-reduce
  LaneCtl* ctl_pm;              // constant {1, -1}
  LaneCtl* ctl_mp;              // constant {-1, 1}
  LaneCtl* ctl_m0;              // constant {-1, 0}: p2 = -A'q2 (two_mixed_device)
  bool craig_x = false;         // FPSQ_CRAIG_X=1: CRAIG carries x through its loop (the recurrence xs += e0 v~) instead of p2 = xsign A'q2 behind it
  int tail_lanes = 3;           // FPSQ_TAIL_LANES=2: fpsq_solve_two_mixed / fpsq_ys_gs form v = -A'q2 and p1 = g - A'q1 by a single-lane product
                                // launch each, not as two lanes of ONE launch (k_spmv_seam)
  bool craig_v_alone = false;   // FPSQ_CRAIG_X=2 (tests): no recurrence, and p2 ALWAYS by the single-lane product k_spmv<1, ..>, never inside a tail launch
  Comm* comm = nullptr;         // null: single GPU
  // Halo mode of the sharded handle (fpsq_comm_set_halo): n is the length of this rank's COLUMN WINDOW; its first
  // `ovl` entries are shared with rank - 1, its last `ovr` with rank + 1; sums over n-vectors run over the owned prefix
  // [0, n - ovr) and are all-reduced like the sums over the (row-sharded) m-vectors.
  bool halo = false;
  int64_t ovl = 0, ovr = 0;
  double* halo_recv = nullptr;  // 2 x [(ovl + ovr)][2]: the neighbours' raw sums on the two overlap regions; consecutive
                                // exchanges alternate between the two halves (a neighbour that is one exchange ahead --
                                // the epilogue runs several without a reduction in between -- never overwrites a record
                                // this rank has not consumed yet)
  uint64_t halo_calls = 0;
  double* halo_raw = nullptr;   // [(ovl + ovr)][2]: this rank's raw sums there (k_spmv<.., HALO>), head region first
  int halo_gf = 0;              // workgroups of k_halo_finish (0: no overlap at all)
  // Halo mode keeps every partial-sum array of the Krylov loop in ONE per-rank segment `seg`, laid out
  //   [E0 | E1 | M0 | M1 | T0 | T1 | V0 | V1 | A0 | A1 | W0 | W1 | E3]
  //   (pE, pE2, pEm[0..1], pS lanes, pWalt[0..1], pS2 lanes, pW[0..1], pE3: the steps behind an A product read the A partials
  //   and ONE half of the update partials -- with a half on either side of A both ranges are contiguous)
  // with counts cE / cW / cT / cA padded to the maxima over the ranks (zeros beyond a rank's own count -- every array is
  // always written with the same local count, so the padding stays zero): the arrays a
  // scalar step reads are then one contiguous range, which is all-gathered into `gath` ([nranks][range]) right before
  // the step; the step kernel sums the ranks' copies itself (StepArgs::nseg).
  double* seg = nullptr;
  double* gath = nullptr;
  int64_t seg_len = 0;
  int cE = 0, cT = 0, cA = 0, cW = 0;
  bool gather_ready = false;
  uint32_t xch_seq = 0;         // sequence number of the last in-launch sum over the ranks (xch_sum; the same on every rank)
  uint32_t last_xseq = 0;       // what prepare_step gave the pair it has just prepared (0: no exchange): travels NEXT to the steps --
  uint32_t ride_xseq = 0;       // k_step's arguments, the RideArgs of the launch whose leaders compute them (pre_args sets ride_xseq)
  uint64_t gather_calls = 0;    // the all-gathers alternate between the two halves of `gath`: a peer that is one reduction
                                // ahead never overwrites a record its neighbour has not read yet
  double* comm_vec = nullptr;   // [n][2] all-reduce payload (partial A' products)
  double* comm_scal = nullptr;  // 8 doubles: scalar all-reduce payload
  double* dscal;               // small device scalar scratch
  Progress* prog_host = nullptr;  // host-mapped
  Progress* prog_dev = nullptr;
  fpsq_stats* hstats = nullptr;   // host-mapped: written by the step kernel that ends a recurrence
  fpsq_stats* hstats_dev = nullptr;
  double* hscal = nullptr;        // host-mapped: scalar results (phi, f, c'c) written by the kernel that computes them
  double* hscal_dev = nullptr;
  // MINRES on K itself (kkt_method = FPSQ_KKT_MINRES_K): allocated at the first call
  bool mk_ready = false;
  MkVecs mk_long{}, mk_short{};
  MinresState* mk_state = nullptr;  // [2]
  double* mk_part[2] = {nullptr, nullptr};
  int mk_gl = 0, mk_gs = 0;
  int64_t expect_iters[5][5][2] = {};  // [kind of lane 0][kind of lane NL-1]: iterations the last two such runs needed
  bool adaptive_runahead = true;    // FPSQ_ADAPTIVE_RUNAHEAD=0 disables (A/B)
  // FPSQ_HOST_TRACE=1: host timestamps at fixed points of fpsq_qp_objgrad, averaged and printed at destroy (developer aid)
  bool host_trace = false;
  double ht_sum[12] = {};
  int64_t ht_calls = 0;
  std::chrono::steady_clock::time_point ht_last, ht_exit;
  bool ht_have_exit = false;
  // stream-ordered outputs (fpsq_set_output_ordering)
  bool out_ordered = false;
  hipEvent_t ev_out = nullptr;
  double call_seq = 0.0;            // sequence number the phi reduction stores behind its results (hscal[3])
  // FPSQ_AB_MASK (developer A/B, tools/ab_modes.py): 1 = gradient kernel not merged into the start-up launch, 2 = final
  // LSQR update not absorbed by k_ys, 4 = phi reduced by a launch of its own right behind k_ys (default: the gradient
  // kernel's extra workgroup), 8 = no stream-ordered return
  int ab_mask = 0;
  bool ab_dynamic = false;          // FPSQ_AB_DYNAMIC=1: the mask is re-read from the environment at every qp_objgrad call
  int64_t force_expect = -1;        // fpsq_debug_expect_iterations: overrides the expected count of the next run (test hook)

  // instrumentation
  bool profile = false;
  std::vector<EventPair> ev_pool;
  size_t ev_used = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::chrono::steady_clock::time_point t_call;
  fpsq_info info{};
  int64_t launches = 0, spmv_launches = 0;
  int64_t prod_a[2] = {0, 0}, prod_at[2] = {0, 0};
};

// The switches a handle reads from the environment ONCE, when it is created (fpsq_create calls this behind its look at the
// device: FPSQ_FUSE_ANY_DEVICE widens what that look allowed).  Read elsewhere: the structure-time ones in finish_structure
// (fpsq_structure.hip.h), FPSQ_REFRESH_SPLIT and a dynamic FPSQ_AB_MASK per call and FPSQ_COMM_ROUTE in fpsq.hip, the
// communicators' own in fpsq_comm.hip.h.  INTEGRATION.md lists every one.
static void read_switches(fpsq_handle h) {
  if (const char* ev = std::getenv("FPSQ_ADAPTIVE_RUNAHEAD")) h->adaptive_runahead = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_HOST_TRACE")) h->host_trace = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_AT_SORTED")) h->at_sorted = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_AT_SHARED")) h->at_shared = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_RIDE_LEAD")) h->ride_lead = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_ATL_TWO")) h->atl_two = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_AT_XCD")) h->at_xcd = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_FUSE_ITER")) h->fuse_iter = std::atoi(ev);
  if (const char* ev = std::getenv("FPSQ_DEBUG_FUSE_BREAK")) h->fuse_break = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_FUSE_HALO")) h->fuse_halo_on = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_MULTI_ITER")) h->multi_max = std::min(std::max(std::atoi(ev), 1), kMultiMax);
  if (const char* ev = std::getenv("FPSQ_MULTI_DEFER_LONG")) h->multi_defer_long = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_MULTI_UPD")) {
    int a = 0, b = 0;
    if (std::sscanf(ev, "%d,%d", &a, &b) == 2 && a >= 8 && b >= 8) {
      h->multi_upd_t = a / 8 * 8;
      h->multi_upd_a = b / 8 * 8;
    }
  }
  if (const char* ev = std::getenv("FPSQ_MINRES_MERGE")) h->minres_merge = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_DEBUG_FUSE_ROTATE")) h->fuse_rotate = std::atoi(ev) & 7;
  if (const char* ev = std::getenv("FPSQ_DEBUG_RIDE_DELAY_MID")) h->ride_delay_mid = std::atoi(ev);
  if (const char* ev = std::getenv("FPSQ_FUSE_PROBE")) {
    h->fuse_probe_path = ev;
    h->fuse_probe_at = 100;
    if (const char* at = std::getenv("FPSQ_FUSE_PROBE_AT")) h->fuse_probe_at = std::atoll(at);
  }
  if (const char* ev = std::getenv("FPSQ_FUSE_TAIL")) h->fuse_tail = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_TAIL_LANES")) h->tail_lanes = std::atoi(ev) == 2 ? 2 : 3;
  if (const char* ev = std::getenv("FPSQ_CRAIG_X")) {
    h->craig_x = std::atoi(ev) == 1;
    h->craig_v_alone = std::atoi(ev) == 2;
  }
  if (const char* ev = std::getenv("FPSQ_ADOPT_STREAM")) h->adopt_streams = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_DEBUG_RIDE_BREAK")) h->ride_break = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_DEBUG_RIDE_DELAY")) h->ride_delay = std::atoi(ev);
  if (const char* ev = std::getenv("FPSQ_JAC_REFRESH")) h->refresh_3pass = std::atoi(ev) == 3;
  if (const char* ev = std::getenv("FPSQ_FUSE_ANY_DEVICE")) h->fuse_hw_ok = h->fuse_hw_ok || std::atoi(ev) != 0;  // (bring-up on other parts)
  if (const char* ev = std::getenv("FPSQ_VERBOSE")) h->verbose = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("FPSQ_AB_MASK")) h->ab_mask = std::atoi(ev);
  if (const char* ev = std::getenv("FPSQ_AB_DYNAMIC")) h->ab_dynamic = std::atoi(ev) != 0;
}

struct fpsq_qp_s {
  fpsq_handle h;
  double *q, *d, *b;
  // fpsq_qp_create_csr only (r_rowptr != null): Q = diag(q) + R, R in CSR with sorted rows; d_eff = d + R x of the current
  // objgrad; `tail`: where the tail writes gx / Hv for the gated launch behind it to subtract R p2 / R (v - p1) from
  int32_t *r_rowptr = nullptr, *r_colind = nullptr;
  double *r_vals = nullptr, *d_eff = nullptr, *tail = nullptr;
  int lgR = 1;             // lanes per row of R (lane_group)
  int gridF = 1, gridR = 1;  // workgroups of the front launch of objgrad (its partials share pQ with the start-up's) / of the others
};

namespace {

#define HIPCHK(h, call)                                                                          \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
      return FPSQ_ERR_HIP;                                                                       \
    }                                                                                            \
  } while (0)

template <class T>
int dalloc(fpsq_handle h, T** p, size_t count) {
  void* q = nullptr;
  HIPCHK(h, hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
  h->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

// a buffer the peers of a sharded handle may write into: allocated the way the communicator needs it (Comm::alloc_exchange)
template <class T>
int xalloc(fpsq_handle h, T** p, size_t count) {
  void* q = nullptr;
  HIPCHK(h, h->comm->alloc_exchange(&q, std::max<size_t>(count, 1) * sizeof(T)));
  h->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

// release one dalloc'ed buffer before the handle dies
template <class T>
void dfree(fpsq_handle h, T** p) {
  auto it = std::find(h->allocs.begin(), h->allocs.end(), (void*)*p);
  if (it != h->allocs.end()) h->allocs.erase(it);
  hipFree(*p);
  *p = nullptr;
}

inline int ew_grid(int64_t n) {
  int64_t g = (n + kBlock - 1) / kBlock;
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, kEwBlocksMax));
}

}  // namespace
