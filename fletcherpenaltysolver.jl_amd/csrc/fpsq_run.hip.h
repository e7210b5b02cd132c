// fpsq_run.hip.h -- the Krylov driver: the lanes' parameters and their start-up kernel, Lane, the step and update launches,
// TailCtx / RunRequest / RunResult, KrylovRun<NL>, run_krylov, run_lanes.
// Part of fpsq.hip's translation unit.
#pragma once

#include "fpsq_launch.hip.h"

#include <algorithm>
#include <functional>
#include <utility>

namespace {

// ------------------------------------------------------------------ Krylov drivers

struct LsqrParams {
  double lambda, atol, rtol, axtol, btol, etol, conlim;
  int64_t itmax;
  int32_t pub_from;
};

__device__ __forceinline__ void lsqr_set_params(LsqrState* S, const LsqrParams& P) {
  S->lambda = P.lambda;
  S->atol = P.atol;
  S->rtol = P.rtol;
  S->axtol = P.axtol;
  S->btol = P.btol;
  S->etol = P.etol;
  S->ctol = P.conlim > 0.0 ? 1.0 / P.conlim : 0.0;
  S->itmax = P.itmax;
  S->pub_from = P.pub_from;
  S->ctl.done = 0;
  S->ctl.skip = 0;
  S->ctl.upd_iter = -1;
}

struct CraigParams {
  double mu, lambda, atol, rtol, btol, conlim, xsign;
  int64_t itmax;
  int32_t start_skipped;
  int32_t pub_from;
};

__device__ __forceinline__ void craig_set_params(CraigState* S, const CraigParams& P) {
  S->mu = P.mu;
  S->lambda = P.lambda;
  S->atol = P.atol;
  S->rtol = P.rtol;
  S->btol = P.btol;
  S->ctol = P.conlim > 0.0 ? 1.0 / P.conlim : 0.0;
  S->xsign = P.xsign;
  S->itmax = P.itmax;
  S->pub_from = P.pub_from;
  S->ctl.done = 0;
  S->ctl.skip = P.start_skipped;  // stays out of the LSQR lane's start-up product; craig_begin clears it
  S->ctl.upd_iter = -1;
}

struct LnlqParams {
  double mu, atol, rtol, xsign;
  int64_t itmax;
  int32_t start_skipped, pub_from;
};

__device__ __forceinline__ void lnlq_set_params(LnlqState* S, const LnlqParams& P) {
  S->mu = P.mu;
  S->atol = P.atol;
  S->rtol = P.rtol;
  S->xsign = P.xsign;
  S->itmax = P.itmax;
  S->pub_from = P.pub_from;
  S->ctl.done = 0;
  S->ctl.skip = P.start_skipped;  // stays out of the LSQR lane's start-up product; lnlq_begin_step clears it
  S->ctl.upd_iter = -1;
}

struct MinresParams {
  double lambda, atol, rtol, etol, conlim;
  int64_t itmax;
  int32_t pub_from;
};

__device__ __forceinline__ void minres_set_params(MinresState* S, const MinresParams& P) {
  S->lambda = P.lambda;
  S->atol = P.atol;
  S->rtol = P.rtol;
  S->etol = P.etol;
  S->ctol = P.conlim > 0.0 ? 1.0 / P.conlim : 0.0;
  S->itmax = P.itmax;
  S->pub_from = P.pub_from;
  S->ctl.done = 0;
  S->ctl.skip = 1;  // stays out of the LSQR lane's start-up product; minres_begin_step clears it
  S->ctl.upd_iter = -1;
  S->ctlT.done = 0;
  S->ctlT.skip = 0;
  S->ctlT.upd_iter = -1;
  S->ctlT.ca = 1.0;  // tmp = A' r2, raw
  S->ctlT.cb = 0.0;
  S->kmode = 0;
  S->kdelta = 0.0;
}

// Start-up of a run in ONE launch: lane parameters (workgroup 0), the right-hand sides loaded into their interleaved
// lanes with the squared-norm partials, and the vectors that start at zero.
struct LoadSeg {
  const double* src;
  double scale;
  double* dst;
  double* dst2;  // optional plain copy of the scaled vector (MINRES keeps r2 = b next to the pair's lane)
  int32_t lane, nblk;
  int64_t len;
  int64_t sum_len;  // the squared-norm partials run over [0, sum_len) (halo mode: the owned prefix of an n-vector)
  double* partials;
};
template <int NL>
__global__ __launch_bounds__(kBlock) void k_startup(LsqrState* S0, LsqrParams P0, LsqrState* S1, LsqrParams P1, CraigState* C,
                                                    CraigParams PC, MinresState* M, MinresParams PM, LnlqState* Q,
                                                    LnlqParams PQ, LoadSeg l0, LoadSeg l1, ZeroArgs z, int nzblk,
                                                    const QpGradArgs qg) {
  __shared__ double red[4];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (S0) lsqr_set_params(S0, P0);
    if (S1) lsqr_set_params(S1, P1);
    if (C) craig_set_params(C, PC);
    if (M) minres_set_params(M, PM);
    if (Q) lnlq_set_params(Q, PQ);
  }
  // qp_objgrad's fast start: the first qg.nblk workgroups evaluate g = q .* x + d, write the long pair {g, x} and the
  // partial sums of f and ||g||^2 (the user-model evaluation of _compute_ys_gs!, model:238-240) -- one launch, no
  // kernel boundary between the model evaluation and the start-up of the recurrences
  if ((int)blockIdx.x < qg.nblk) {
    qp_grad_body(qg, blockIdx.x, red);
    return;
  }
  int blk = blockIdx.x - qg.nblk;
  if (blk < l0.nblk + l1.nblk) {
    const bool first = blk < l0.nblk;
    if (!first) blk -= l0.nblk;
    const double* src = first ? l0.src : l1.src;
    double* dst = first ? l0.dst : l1.dst;
    double* dst2 = first ? l0.dst2 : l1.dst2;
    const double scale = first ? l0.scale : l1.scale;
    const int lane = first ? l0.lane : l1.lane;
    const int nb = first ? l0.nblk : l1.nblk;
    const int64_t len = first ? l0.len : l1.len;
    const int64_t sum_len = first ? l0.sum_len : l1.sum_len;
    double* partials = first ? l0.partials : l1.partials;
    double sq = 0.0;
    for (int64_t i = (int64_t)blk * kBlock + threadIdx.x; i < len; i += (int64_t)nb * kBlock) {
      const double v = scale * src[i];
      dst[i * NL + lane] = v;
      if (dst2) dst2[i] = v;
      if (i < sum_len) sq += v * v;
    }
    const double t = block_sum(sq, red);
    if (threadIdx.x == 0) partials[blk] = t;
    return;
  }
  blk -= l0.nblk + l1.nblk;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!z.p[k]) continue;
    for (int64_t i = (int64_t)blk * kBlock + threadIdx.x; i < z.n[k]; i += (int64_t)nzblk * kBlock) z.p[k][i] = 0.0;
  }
}

enum { LANE_LSQR = 1, LANE_CRAIG = 2, LANE_MINRES = 3, LANE_LNLQ = 4 };
// the two least-norm recurrences share their vector plumbing (short Mu~, w, y; long v~, x)
inline bool is_ln(int kind) { return kind == LANE_CRAIG || kind == LANE_LNLQ; }

// One Krylov recurrence of a (possibly fused) run.
struct Lane {
  int kind = 0;
  const double* rhs = nullptr;  // LSQR: n-vector b;  CRAIG, MINRES: m-vector b
  double rhs_scale = 1.0;
  double lambda = 0.0;          // LSQR regularisation; MINRES: shift of A A' + lambda I
  double delta = 0.0;           // CRAIG: M = (1/delta) I, sqd when != 0
  double xsign = 1.0;           // CRAIG: xs accumulates xsign * x
  double* x = nullptr;          // LSQR, MINRES: solution (m).  CRAIG: xs (n); null: x is not carried through the loop -- the
                                //   caller forms xs = xsign A'y from the final y (two_mixed_device)
  double* y = nullptr;          // CRAIG: y (m)
  fpsq_stats* st = nullptr;     // destination of the final stats: an element of the host-mapped h->hstats
  fpsq_stats* st_dev = nullptr; // its device alias (filled by run_krylov / run_minres)
  // fast start (qp_objgrad, fused single-GPU runs):
  bool preloaded = false;               // LSQR: the caller already wrote rhs into the long pair's lane and ||rhs||^2 partials to pE
  const double* affine_shift = nullptr; // CRAIG: rhs = -(A z - shift) with z already in the long pair's lane: formed by the
  double* affine_out = nullptr;         //        LSQR start-up product (the lane is otherwise parked there); A z - shift -> affine_out
  // filled by run_krylov
  void* state = nullptr;
  void* state_alt = nullptr;    // the other copy of the state (riding steps alternate between the two)
  void* state_alt2 = nullptr;   // a third one (fused iterations: the step behind the A' product lands there, see k_iter_fused)
  LaneCtl* ctl = nullptr;       // coefficients of the A product (and of the A' product for LSQR / CRAIG)
  LaneCtl* ctlT = nullptr;      // coefficients of the A' product (MINRES: the raw tmp = A' r2)
  int64_t itmax = 0;
};

StepArgs step_args(int kind, const Lane& L, int it, const double* p0, int n0, const double* p1, int n1, Progress* prog) {
  StepArgs a{};
  a.kind = kind;
  a.it = it;
  a.state = L.state;
  a.p0 = p0;
  a.p1 = p1;
  a.n0 = n0;
  a.n1 = n1;
  a.prog = prog;
  a.host_stats = L.st_dev;
  return a;
}

void launch_step_raw(fpsq_handle h, const StepArgs& a0, const StepArgs& a1, uint32_t xseq = 0) {
  const int nb = a1.kind != STEP_NONE ? 2 : 1;
  const XchTable* xt = xseq ? insum_table(h) : nullptr;
  if (xt) hipLaunchKernelGGL(k_step<true>, dim3(nb), dim3(kStepThreads), 0, h->stream, a0, a1, xt, (unsigned int)xseq);
  else hipLaunchKernelGGL(k_step<false>, dim3(nb), dim3(kStepThreads), 0, h->stream, a0, a1, xt, 0u);
  h->launches++;
}

// `sharded`: the partial arrays of these steps are sums over m-vectors, of which a rank only holds its rows:
// local sums -> one scalar all-reduce (4 doubles) -> the step kernel reads the global sums.
// padded (common to all ranks) count of the segment array that starts at p; 0: not an array of the segment
int seg_count(fpsq_handle h, const double* p) {
  if (p == h->pE || p == h->pE2) return h->cE;
  if (p == h->pEm[0] || p == h->pEm[1]) return h->cW;
  if (p == h->pS || p == h->pS + h->strT) return h->cT;
  if (p == h->pS2 || p == h->pS2 + h->strA) return h->cA;
  if (p == h->pW[0] || p == h->pW[1] || p == h->pWalt[0] || p == h->pWalt[1] || p == h->pE3) return h->cW;
  return 0;
}

// Everything a step needs BEFORE its kernel: row-sharded runs gather (halo mode) or pre-sum + all-reduce the partial sums
// its arguments point to, and the arguments are redirected to the gathered / reduced numbers.  A step that rides in the next
// product launch is prepared when it is handed over (the collective must precede that launch in the stream).
int prepare_step(fpsq_handle h, StepArgs& a0, StepArgs& a1, bool sharded = false, int sharded1 = -1) {
  const bool sh[2] = {sharded, sharded1 < 0 ? sharded : sharded1 != 0};  // per step: its partials are per-rank sums
  h->last_xseq = 0;
  if (h->comm && h->halo && insum(h)) {
    // the step's workgroup forms the sum over the ranks itself (xch_sum): the arguments stay the rank's local arrays, and the pair
    // gets an exchange number -- the same sequence on every rank -- which travels next to the steps (h->last_xseq: the caller
    // hands it to k_step or to the launch whose leaders compute the pair).  A communicator of one: nothing at all.
    if (insum_table(h) != nullptr && ((sh[0] && a0.kind != STEP_NONE) || (sh[1] && a1.kind != STEP_NONE))) h->last_xseq = next_xseq(h);
    return 0;
  }
  if (h->comm && h->halo && (sh[0] || sh[1])) {
    // Halo mode: ONE all-gather of the contiguous segment range holding the arrays these steps read; the step kernel then
    // sums the nranks copies of every array in rank-major order (no local pre-sum launch, no reduction by the library).
    StepArgs* w[2] = {&a0, &a1};
    const double *lo = nullptr, *hi = nullptr;
    for (int k = 0; k < 2; ++k) {
      if (w[k]->kind == STEP_NONE || !sh[k]) continue;
      const double* ps[2] = {w[k]->p0, w[k]->p1};
      for (const double* q : ps) {
        if (!q) continue;
        const int c = seg_count(h, q);
        if (c == 0) {
          h->err = "internal: a sharded step reads a partial array outside the gather segment";
          return FPSQ_ERR_STATE;
        }
        if (!lo || q < lo) lo = q;
        if (!hi || q + c > hi) hi = q + c;
      }
    }
    const int64_t len = hi - lo;
    double* gbuf = h->gath + (size_t)(h->gather_calls++ & 1) * (size_t)h->seg_len * h->comm->nranks;
    if (int rc = h->comm->allgather(lo, gbuf, (size_t)len, h->stream)) {
      h->err = h->comm->err;
      return rc;
    }
    for (int k = 0; k < 2; ++k) {
      if (w[k]->kind == STEP_NONE || !sh[k]) continue;
      w[k]->n0 = seg_count(h, w[k]->p0);
      w[k]->p0 = gbuf + (w[k]->p0 - lo);
      if (w[k]->p1) {
        w[k]->n1 = seg_count(h, w[k]->p1);
        w[k]->p1 = gbuf + (w[k]->p1 - lo);
      }
      w[k]->nseg = h->comm->nranks;
      w[k]->seg_stride = (int32_t)len;
    }
    return 0;
  }
  if (h->comm && (sh[0] || sh[1])) {
    PresumArgs P{};
    const StepArgs* a[2] = {&a0, &a1};
    for (int k = 0; k < 2; ++k) {
      if (a[k]->kind == STEP_NONE || !sh[k]) continue;
      P.p[2 * k] = a[k]->p0;
      P.n[2 * k] = a[k]->n0;
      P.p[2 * k + 1] = a[k]->p1;
      P.n[2 * k + 1] = a[k]->n1;
    }
    hipLaunchKernelGGL(k_presum, dim3(1), dim3(kBlock), 0, h->stream, P, h->comm_scal);
    h->launches++;
    if (int rc = comm_allreduce(h, h->comm_scal, 4)) return rc;
    StepArgs* w[2] = {&a0, &a1};
    for (int k = 0; k < 2; ++k) {
      if (w[k]->kind == STEP_NONE || !sh[k]) continue;
      w[k]->p0 = h->comm_scal + 2 * k;
      w[k]->n0 = 1;
      if (w[k]->p1) {
        w[k]->p1 = h->comm_scal + 2 * k + 1;
        w[k]->n1 = 1;
      }
    }
  }
  return 0;
}

int launch_step(fpsq_handle h, StepArgs a0, StepArgs a1, bool sharded = false, int sharded1 = -1) {
  if (int rc = prepare_step(h, a0, a1, sharded, sharded1)) return rc;
  launch_step_raw(h, a0, a1, h->last_xseq);
  return 0;
}

template <int NL>
void launch_updates(fpsq_handle h, const UpdSeg& s0, const UpdSeg& s1, const UpdSeg& s2) {
  const int nb = s0.nblk + s1.nblk + s2.nblk;
  if (nb == 0) return;
  hipLaunchKernelGGL(k_updates<NL>, dim3(nb), dim3(kBlock), 0, h->stream, s0, s1, s2);
  h->launches++;
}


// Runs 1 or 2 recurrences in lock-step on the interleaved Golub-Kahan pairs LP (n) / SP (m):
//   A' product: LP <- ca A' SP + cb LP      (LSQR: u~ <- B v - alpha u;     CRAIG: v~ <- B'u - beta v)
//   A  product: SP <- ca A  LP + cb SP      (LSQR: v~ <- B'u - beta v;      CRAIG: Mu~ <- B v - alpha Mu)
// Each lane is exactly Krylov.jl's lsqr! / craig! on its own right-hand side (its results do not depend on the
// other lane); running them side by side turns two SpMVs into one SpMM with k = 2.
// `tail` (optional, single GPU): enqueues the caller's epilogue kernels.  When the iteration count of the previous call
// of the same kind is known, the final LSQR flush and the tail are enqueued SPECULATIVELY right behind iteration
// `expect`, gated on the lanes' `done` flags (TailCtx::gates): if the recurrences do end there -- consecutive evaluations of
// a line search mostly repeat their counts -- the epilogue runs without the host first having to see `done` and only
// then launching it (a ~30 us bubble per evaluation); if not, the gated kernels exit at once and the loop goes on.
// RunResult::tail_was_run tells the caller whether its epilogue has been taken care of.
//
// Structure (round 4; one 640-line function before): KrylovRun::run() is the loop and knows three things -- a PRODUCT is
// launched (with whatever rides in it), the STEPS behind it are posted (PendingSteps: they ride in the next product launch
// or get a launch of their own), the host PACES itself (exchange boundaries of a sharded run, run-ahead, speculation).
// What a recurrence of a given kind contributes at each of those points -- which step kinds, which update segments,
// which partial arrays -- is in the builders (lane_*, *_seg, steps_after_*); nothing outside them switches on a lane's kind.
struct TailCtx {
  Gates gates;                // the speculative epilogue's gates (none: the epilogue runs after the loop)
  UpdSeg flush = seg_none();  // the final LSQR x update, left to the epilogue's first kernel (k_ys; UPD_NONE: none)
};
using TailFn = std::function<int(const TailCtx&)>;

// What the caller asks of one run beyond its lanes (qp_objgrad's fast start)
struct RunRequest {
  QpGradArgs startup_qg{};    // nblk > 0: the start-up launch of the run also evaluates the eq-QP gradient
  // The final LSQR x update may be left to the caller's epilogue when its FIRST kernel is k_ys: the run then parks the
  // segment in the TailCtx (or in RunResult::flush) instead of launching it.
  bool absorb_flush = false;
};

// ... and what the caller needs from it afterwards
struct RunResult {
  bool tail_was_run = false;  // the caller's epilogue was enqueued (gated) inside the run and the gates were open
  UpdSeg flush = seg_none();  // otherwise: the final LSQR x update the epilogue has to apply (absorb_flush)
};

// ---- what depends on the KIND of a recurrence
inline int lane_begin_kind(const Lane& L) {
  return L.kind == LANE_LSQR ? STEP_LSQR_BEGIN : L.kind == LANE_CRAIG ? STEP_CRAIG_BEGIN : L.kind == LANE_LNLQ ? STEP_LNLQ_BEGIN : STEP_MINRES_BEGIN;
}
// the step behind the A' product of an iteration (a MINRES lane runs the stopping tests of the previous iteration there)
inline int lane_kind_after_at(const Lane& L) {
  return L.kind == LANE_LSQR ? STEP_LSQR_SA : L.kind == LANE_CRAIG ? STEP_CRAIG_SA : L.kind == LANE_LNLQ ? STEP_LNLQ_SA : STEP_MINRES_C;
}
// ... and behind the A product (MINRES: step A, between its stages E1 and E2)
inline int lane_kind_after_a(const Lane& L) {
  return L.kind == LANE_LSQR ? STEP_LSQR_SB : L.kind == LANE_CRAIG ? STEP_CRAIG_SB : L.kind == LANE_LNLQ ? STEP_LNLQ_SB : STEP_MINRES_A;
}
inline const int32_t* lane_iter_ptr(const Lane& L) {
  return L.kind == LANE_LSQR ? &((LsqrState*)L.state)->iter
         : L.kind == LANE_CRAIG ? &((CraigState*)L.state)->iter
         : L.kind == LANE_LNLQ  ? &((LnlqState*)L.state)->iter
                                : &((MinresState*)L.state)->iter;
}
// a MINRES / LNLQ lane reports iteration k (step C; pass k) while the host is enqueueing iteration k + 1
inline int lane_lag(const Lane& L) { return L.kind == LANE_MINRES || L.kind == LANE_LNLQ ? 1 : 0; }
// after a product launch that carried the lane's step: the lane lives in its other state copy now
inline void lane_swap_state(Lane& L) {
  std::swap(L.state, L.state_alt);
  L.ctl = reinterpret_cast<LaneCtl*>(L.state);  // LaneCtl is the first member of every state
  L.ctlT = L.kind == LANE_MINRES ? &reinterpret_cast<MinresState*>(L.state)->ctlT : L.ctl;
}

template <int NL>
struct KrylovRun {
  fpsq_handle h;
  Lane* lanes;
  const TailFn* tail;
  const RunRequest req;
  RunResult res;
  const int64_t n, m;
  const fpsq_options& o;
  hipStream_t s;
  const int gn, gm, nbA;
  double *LP, *SP;
  double* LPalt = nullptr;  // the second long pair (several iterations per launch alternate; nullptr: not available)
  bool can_multi = false;   // ... whenever the previous product's steps are pending and the expected count leaves room for >= 2
  // the run-ahead's expectation (see run())
  int64_t* expect_slot;
  const bool local_vec;    // vector updates touch rank-local data only (one GPU, or the halo-sharded layout)
  int64_t expect = 0;
  int32_t pub_from = 0;
  // the lanes
  bool any_lsqr = false;
  int64_t itmax_all = 0;
  Progress* prog[2] = {nullptr, nullptr};
  int minres_lane = -1, affine_lane = -1;
  LsqrState* lsS[2] = {nullptr, nullptr};
  LsqrParams lsP[2] = {};
  CraigState* crS = nullptr;
  CraigParams crP{};
  MinresState* mrS = nullptr;
  MinresParams mrP{};
  LnlqState* lqS = nullptr;
  LnlqParams lqP{};
  bool lead = false;        // the steps ride in the next product launch (leader workgroups)
  bool fuse_upd = false;    // the vector updates ride in the product launches
  bool split_steps = false; // replicated n-sums and per-rank m-sums cannot share a presum launch
  bool can_fuse = false;    // a joint iteration is ONE launch (k_iter_fused) whenever the previous product's steps are pending
  // Where the last A product left its squared-norm partials.  A fused launch READS them (head leaders; mid leaders redoing the
  // head step, any of which another kernel may hold up) while its own row groups -- released per XCC -- WRITE theirs: the
  // launch writes the other array (found by test_one_launch_iterations_with_a_late_mid_leader, which fails with one array)
  double* pa_last = nullptr;
  StepArgs none{};
  // the steps behind the last product, not launched yet
  StepArgs pend[2];
  bool have_pend = false;
  uint32_t pend_xseq = 0;  // ... and the number of their exchange (sharded, in-launch sums; 0: none)
  // the loop
  double *SPcur, *SPalt;
  int look = 1;
  int64_t it = 0;
  int64_t spec_it = -1;  // iteration behind which the gated flush + tail were enqueued
  int64_t tail_launches = 0;
  UpdSeg winit[2] = {seg_none(), seg_none()};
  UpdSeg lu[2] = {seg_none(), seg_none()};  // what rides in (or precedes) this iteration's products: LSQR's update of the previous one
  int nlu = 0;

  KrylovRun(fpsq_handle h_, Lane* lanes_, const TailFn* tail_, const RunRequest& req_)
      : h(h_), lanes(lanes_), tail(tail_), req(req_), n(h_->n), m(h_->m), o(h_->opt), s(h_->stream), gn(ew_grid(h_->n)), gm(ew_grid(h_->m)),
        nbA(npart_A(h_)), LP(h_->LP), SP(h_->SP), expect_slot(h_->expect_iters[lanes_[0].kind][lanes_[NL - 1].kind]),
        local_vec(!h_->comm || h_->halo), SPcur(h_->SP), SPalt(h_->SP2) {
    none.kind = STEP_NONE;
  }

  // coefficients of the A product / the A' product
  LaneCtl* c0() const { return lanes[0].ctl; }
  LaneCtl* c1() const { return lanes[NL - 1].ctl; }
  LaneCtl* t0() const { return lanes[0].ctlT; }
  LaneCtl* t1() const { return lanes[NL - 1].ctlT; }

  // ------------------------------------------------------------------ set-up of the lanes
  void setup() {
    // iteration count of the previous runs with the same pair of recurrences (0: unknown).  The scalar steps publish their
    // progress to the host only from that iteration on (and when a recurrence ends): see publish().
    // (sharded: only in halo mode, where every rank derives the same count from the replicated recurrence state)
    // The LARGER of the last two counts.  The two ways of being wrong cost very differently: one iteration too many is two
    // launches that exit at their first instruction (~7 us); one too few is a speculative epilogue enqueued for nothing, a host
    // round trip before the loop goes on and another before the epilogue is enqueued again (measured with evaluations
    // alternating between a 14- and a 15-iteration regime, bench.py --alternate-delta: +11 % per evaluation when the last
    // count alone is the expectation, profiles/r04_alternate_delta.txt).
    int64_t expect_v = (h->adaptive_runahead && local_vec) ? std::max(expect_slot[0], expect_slot[1]) : 0;
    if (h->force_expect >= 0 && local_vec) expect_v = h->force_expect;
    h->force_expect = -1;
    expect = expect_v;
    pub_from = (int32_t)std::min<int64_t>(expect, INT32_MAX);
    int nlsqr = 0;
    for (int l = 0; l < NL; ++l) {
      Lane& L = lanes[l];
      prog[l] = &h->prog_dev[l];
      h->prog_host[l].iter = 0;
      h->prog_host[l].done = 0;
      L.st_dev = h->hstats_dev + (L.st - h->hstats);
      *L.st = fpsq_stats{};
      if (L.kind == LANE_LSQR) {
        any_lsqr = true;
        LsqrState* S = h->lsqr[nlsqr];
        L.state_alt2 = reinterpret_cast<LsqrState*>(h->state3[0]) + nlsqr;
        L.state_alt = h->lsqr_alt[nlsqr++];
        L.state = S;
        L.ctl = &S->ctl;
        L.itmax = o.ls_itmax == 0 ? n + m : o.ls_itmax;
        lsP[nlsqr - 1] = LsqrParams{L.lambda, o.ls_atol, o.ls_rtol, o.ls_axtol, o.ls_btol, o.ls_etol, o.ls_conlim, L.itmax,
                                    pub_from};
        lsS[nlsqr - 1] = S;
      } else if (L.kind == LANE_MINRES) {
        MinresState* S = h->minres;
        L.state_alt = h->minres_alt;
        L.state = S;
        L.ctl = &S->ctl;
        L.ctlT = &S->ctlT;
        L.itmax = o.ne_itmax == 0 ? 2 * m : o.ne_itmax;
        // (its stopping tests of iteration k run one product later than the other recurrences': see the main loop)
        mrP = MinresParams{L.lambda, o.ne_atol, o.ne_rtol, o.ne_etol, o.ne_conlim, L.itmax, std::max(pub_from - 1, 0)};
        mrS = S;
        minres_lane = l;
      } else if (L.kind == LANE_LNLQ) {
        LnlqState* S = h->lnlq;
        L.state_alt = h->lnlq_alt;
        L.state_alt2 = h->state3[2];
        L.state = S;
        L.ctl = &S->ctl;
        // pass k of lnlq!'s loop is completed (and tested) by the step after the A' product of iteration k + 1
        L.itmax = (o.ln_itmax == 0 ? n + m : o.ln_itmax) + 1;
        lqP = LnlqParams{L.delta != 0.0 ? 1.0 / L.delta : 1.0, o.ln_atol, o.ln_rtol, L.xsign, L.itmax - 1, NL == 2 ? 1 : 0,
                         std::max(pub_from - 1, 0)};
        lqS = S;
      } else {
        CraigState* S = h->craig;
        L.state_alt = h->craig_alt;
        L.state_alt2 = h->state3[1];
        L.state = S;
        L.ctl = &S->ctl;
        L.itmax = o.ln_itmax == 0 ? n + m : o.ln_itmax;
        const bool reg = L.delta != 0.0;
        crP = CraigParams{reg ? 1.0 / L.delta : 1.0, reg ? 1.0 : 0.0, o.ln_atol, o.ln_rtol, o.ln_btol, o.ln_conlim,
                          L.xsign, L.itmax, NL == 2 ? 1 : 0, pub_from};
        crS = S;
      }
      if (!L.ctlT) L.ctlT = L.ctl;
      itmax_all = std::max(itmax_all, L.itmax);
    }
    // Riding steps (two LSQR / CRAIG lanes; one GPU or the halo-sharded layout): instead of a one-workgroup k_step launch
    // behind every product, the two steps are handed to the NEXT product launch, where leader workgroups compute them and the
    // others pick the coefficients up on their way to the row epilogue (k_spmv_atl, k_spmv_rgcs<.., LEAD>).  Such a step reads
    // the lane's current state copy and writes the other one; the lane's pointers (state, ctl) switch to it once the launch
    // is enqueued.
    lead = NL == 2 && (!h->comm || h->halo) && h->ride_lead && h->AT.padded && (h->AT.sorted || h->AT.col16) && h->RA.ok;
    // (a MINRES lane -- solve_two_extras -- on one GPU only: its sums run over row-sharded m-vectors)
    for (int l = 0; l < NL; ++l)
      lead = lead && (lanes[l].kind == LANE_LSQR || is_ln(lanes[l].kind) || (lanes[l].kind == LANE_MINRES && !h->comm));
    // fast start: the CRAIG lane whose right-hand side the LSQR start-up product forms
    for (int l = 0; l < NL; ++l)
      if (is_ln(lanes[l].kind) && lanes[l].affine_shift && any_lsqr && NL == 2 && local_vec) affine_lane = l;
    // Single GPU: the vector updates ride in the product launches (run_fused_updates).  An update may only read what
    // its host product reads: the LSQR x/w update of iteration it-1 (reads the short pair) goes with the A' product of
    // iteration it; CRAIG's updates of iteration it (read the long pair and the OLD short pair) go with the A product,
    // which therefore writes the alternate short pair (ping-pong).  The same holds for a row-sharded handle in halo mode
    // (every vector a rank updates is its own).  Sharded with replicated n-vectors: separate update launch, in place.
    fuse_upd = local_vec;
    split_steps = h->comm && !h->halo;
    pa_last = h->pS2;
    // (a halo-sharded handle: when its sums over the ranks need no launch of their own and -- for now -- no row of its window is
    // shared with a neighbour: a communicator of one, a block-diagonal Jacobian)
    can_fuse = NL == 2 && h->fuse_ok && h->at_xcd && lead && fuse_upd && minres_lane < 0 && !h->ride_break &&
               (!h->comm || (h->halo && insum(h) && (h->ovl + h->ovr == 0 || (h->fuse_halo_ok && h->fuse_halo_on))));
    look = std::max(1, o.lookahead);
    // several iterations per launch: LSQR / CRAIG lanes of a single-GPU handle whose iterations may share a launch at all
    can_multi = can_fuse && !h->comm && h->multi_ok && h->multi_max > 1 && h->fuse_probe_at == 0;
    for (int l = 0; l < NL; ++l) can_multi = can_multi && (lanes[l].kind == LANE_LSQR || lanes[l].kind == LANE_CRAIG);
    LPalt = can_multi ? h->LP2 : nullptr;
    if (can_multi) hipMemsetAsync(h->mz_hdone, 0, 8, s);  // (nobody has ended yet)
  }

  // ------------------------------------------------------------------ the steps behind a product
  // hands the pending steps to a stand-alone launch (needed whenever the host or a gated kernel must see their effect now)
  int flush_pend(bool sharded) {
    if (!have_pend) return 0;
    have_pend = false;
    if (h->comm) {  // (prepared -- gathered, or numbered -- when they were handed over)
      launch_step_raw(h, pend[0], pend[1], pend_xseq);
      return 0;
    }
    return launch_step(h, pend[0], pend[1], sharded);
  }
  // after a product launch that carried the pending steps: the lanes live in their other state copies now
  void adopt_pend() {
    for (int l = 0; l < NL; ++l)
      if (pend[l].kind != STEP_NONE) lane_swap_state(lanes[l]);
    have_pend = false;
  }
  // the steps behind a product: riding in the next product launch when both lanes have one, else their own launch now
  int post_step(const StepArgs& a0, const StepArgs& a1, bool sharded) {
    if (lead && a0.kind != STEP_NONE && a1.kind != STEP_NONE) {
      pend[0] = a0;
      pend[1] = a1;
      pend_xseq = 0;
      if (h->comm) {
        if (int rc = prepare_step(h, pend[0], pend[1], sharded)) return rc;
        pend_xseq = h->last_xseq;
      }
      have_pend = true;
      return 0;
    }
    return launch_step(h, a0.kind ? a0 : a1, a0.kind ? a1 : none, sharded);
  }
  // the pending steps as the next product launch takes them (null: nothing pending)
  const StepArgs* pre_args(bool for_at) {
    h->ride_xseq = have_pend ? pend_xseq : 0;  // (the launch that takes the steps also takes their exchange's number: launch_spmv)
    if (!have_pend) return nullptr;
    for (int l = 0; l < NL; ++l) {
      pend[l].state = lanes[l].state;
      pend[l].state_out = lanes[l].state_alt;
      pend[l].prod_ctl_off = for_at && lanes[l].kind == LANE_MINRES ? (int32_t)(offsetof(MinresState, ctlT) / 8) : 0;
    }
    return pend;
  }

  // ------------------------------------------------------------------ builders: update segments and step arguments
  // Where the vector update of iteration k leaves its squared-norm partials (read by the step behind the NEXT A product):
  // halves alternate, because the A' launch of iteration k + 1 carries both that step -- riding, computed by sixteen
  // leaders of which any may be late -- and the update of iteration k + 1, whose workgroups only wait for the record of
  // their own XCC's leader before they write.  (CRAIG's update rides one launch later than the step that reads its
  // partials and would be safe in one array; it follows the same parity so that a sharded step gathers one range.)
  double* upd_part(int l, int64_t k) const { return (k & 1) ? h->pWalt[l] : h->pW[l]; }
  UpdSeg lsqr_upd_seg(int l, int64_t it_of_update) const {
    UpdSeg u{};
    u.kind = UPD_LSQR;
    u.it = (int)it_of_update;
    u.ctl = lanes[l].ctl;
    u.src = SPcur;
    u.lane = l;
    u.nblk = gm;
    u.a = lanes[l].x;
    u.b = h->Lw[l];
    u.len = m;
    u.partials = upd_part(l, it_of_update);
    return u;
  }
  UpdSeg lsqr_winit_seg(int l) const {  // w_1 = v_1, x_0 = 0
    UpdSeg u{};
    u.kind = UPD_LSQR_WINIT;
    u.it = 0;
    u.ctl = lanes[l].ctl;
    u.src = SP;
    u.lane = l;
    u.nblk = gm;
    u.a = lanes[l].x;
    u.b = h->Lw[l];
    u.len = m;
    u.partials = upd_part(l, 0);
    return u;
  }
  // the least-norm lane's updates of iteration `it`: long (x, w2) and short (w, y)
  void ln_upd_segs(int l, UpdSeg& lng, UpdSeg& sht) const {
    const Lane& L = lanes[l];
    UpdSeg u{};
    u.kind = L.kind == LANE_LNLQ ? UPD_LNLQ_LONG : L.delta != 0.0 ? UPD_CRAIG_LONG_REG : UPD_CRAIG_LONG;
    u.it = (int)it;
    u.ctl = L.ctl;
    u.src = LP;
    u.lane = l;
    u.nblk = gn;
    u.a = L.x;
    u.b = h->Cw2;
    u.len = n;
    // CRAIG without x in the loop (Lane::x null): nothing long rides -- w2 only ever feeds x
    lng = L.kind == LANE_CRAIG && L.x == nullptr ? seg_none() : u;
    UpdSeg v{};
    v.kind = L.kind == LANE_LNLQ ? UPD_LNLQ_SHORT : UPD_CRAIG_SHORT;
    v.it = (int)it;
    v.ctl = L.ctl;
    v.src = SPcur;
    v.lane = l;
    v.nblk = gm;
    v.a = h->Cw;
    v.b = L.y;
    v.len = m;
    v.partials = upd_part(l, it - 1);
    sht = v;
  }
  // MINRES stage segments of iteration `k` (the Lanczos vector under construction sits in lane l of `pair`)
  UpdSeg minres_seg(int stage, int64_t k, double* pair) const {
    const int l = minres_lane;
    UpdSeg u{};
    u.kind = stage == 1 ? UPD_MINRES_E1 : stage == 2 ? UPD_MINRES_E2 : UPD_MINRES_E3;
    u.it = (int)k;
    u.ctl = lanes[l].ctl;
    u.src = pair;
    u.lane = l;
    u.nblk = gm;
    u.len = m;
    double* r2 = h->Mr[k % 2];
    double* r1 = h->Mr[(k + 1) % 2];  // also receives the new r2
    double* w1 = h->Mw[k % 2];        // w_{k-2}, overwritten by w_k
    double* w2 = h->Mw[(k + 1) % 2];
    if (stage == 1) {
      u.a = r1;
      u.b = r2;
      u.partials = h->pE3;
    } else if (stage == 2) {
      u.a = r2;
      u.b = r1;
      u.c = w2;
      u.d = w1;
      u.partials = h->pW[l];
    } else {
      u.a = w1;
      u.b = lanes[l].x;
      u.partials = h->pWalt[l];  // (rides in the launch whose leaders compute step B from E2's partials in pW[l])
    }
    return u;
  }
  StepArgs minres_step(int kind, int64_t k) const {  // B: after E2 (partials in pW); C: after E3 (partials in pWalt)
    const int l = minres_lane;
    return step_args(kind, lanes[l], (int)k, kind == STEP_MINRES_C ? h->pWalt[l] : kind == STEP_MINRES_A ? h->pE3 : h->pW[l], gm,
                     nullptr, 0, prog[l]);
  }
  // lane l's step behind the A' product of iteration `it` (npT partials per lane)
  StepArgs step_after_at(int l, int npT) const {
    const Lane& L = lanes[l];
    if (L.kind == LANE_MINRES) return it > 1 ? minres_step(STEP_MINRES_C, it - 1) : none;  // the stopping tests of iteration it - 1
    return step_args(lane_kind_after_at(L), L, (int)it, h->pS + (size_t)l * h->strT, npT, nullptr, 0, prog[l]);
  }
  // ... and behind the A product
  StepArgs step_after_a(int l) const {
    const Lane& L = lanes[l];
    if (L.kind == LANE_MINRES) return minres_step(STEP_MINRES_A, it);
    return step_args(lane_kind_after_a(L), L, (int)it, pa_last + (size_t)l * h->strA, nbA,
                     L.kind == LANE_LNLQ ? nullptr : upd_part(l, it - 1), gm, prog[l]);
  }
  bool all_done() const {
    for (int l = 0; l < NL; ++l)
      if (!load_progress(&h->prog_host[l]).done) return false;
    return true;
  }

  // ------------------------------------------------------------------ start-up
  // parameters, right-hand sides, beta_1 (one launch), then (LSQR) alpha_1 and w_1
  int startup() {
    StepArgs b0 = none, b1 = none;
    LoadSeg ld[2] = {};
    ZeroArgs z{};
    int nzblk = 0;
    for (int l = 0; l < NL; ++l) {
      Lane& L = lanes[l];
      double* pe = L.kind == LANE_LSQR ? (l == 0 ? h->pE : h->pE2) : h->pEm[l];
      LoadSeg& g = ld[l];
      g.src = L.rhs;
      g.scale = L.rhs_scale;
      g.lane = l;
      g.partials = pe;
      if (L.kind == LANE_LSQR) {
        // x = 0 is written by the w_1 start-up update (also when the recurrence ends at start-up)
        g.dst = LP;
        g.len = n;
        g.sum_len = n_owned(h);
        g.nblk = L.preloaded ? 0 : gn;  // fast start: the caller wrote the lane and the ||rhs||^2 partials already
        (l == 0 ? b0 : b1) = step_args(STEP_LSQR_BEGIN, L, 0, pe, gn, nullptr, 0, prog[l]);
      } else if (L.kind == LANE_MINRES) {
        // r1 = r2 = b: r2 sits in Mr[1] (iteration 1 reads r2 from Mr[it % 2]) and in the short pair's lane
        g.dst = SP;
        g.dst2 = h->Mr[1];
        g.len = m;
        g.sum_len = m;
        g.nblk = gm;
        z.p[0] = L.x;
        z.p[1] = h->Mw[0];
        z.p[2] = h->Mw[1];
        z.p[3] = h->Mr[0];
        z.n[0] = z.n[1] = z.n[2] = z.n[3] = m;
        nzblk = gm;
      } else {
        if (L.affine_shift) {  // fast start: the lane receives `shift`; the start-up product turns it into -(A z - shift)
          g.src = L.affine_shift;
          g.scale = 1.0;
        }
        g.dst = SP;
        g.len = m;
        g.sum_len = m;
        g.nblk = gm;
        z.p[1] = L.y;
        z.n[1] = m;
        z.p[2] = h->Cw;
        z.n[2] = m;
        nzblk = gm;
        if (L.x != nullptr) {  // (the long recurrence: x, and w2 when regularised)
          z.p[0] = L.x;
          z.n[0] = n;
          if (L.delta != 0.0) {
            z.p[3] = h->Cw2;
            z.n[3] = n;
          }
          nzblk = gn;
        }
      }
    }
    ht_mark(h, 3);
    hipLaunchKernelGGL(k_startup<NL>, dim3(req.startup_qg.nblk + ld[0].nblk + ld[1].nblk + nzblk), dim3(kBlock), 0, s, lsS[0],
                       lsP[0], lsS[1], lsP[1], crS, crP, mrS, mrP, lqS, lqP, ld[0], ld[1], z, nzblk, req.startup_qg);
    h->launches++;
    bool ln_begun = false, minres_begun = false;
    if (any_lsqr) {
      // v~_1 = B'u_1 = A u~_1 / beta_1 for the LSQR lanes.  The CRAIG lane is parked by ctl.skip -- unless its
      // right-hand side is still to be formed (fast start): then it rides along with the constant pair (-1, +1):
      // SP[.][l] <- -A z + shift, and the norm partials of the launch are those of its right-hand side.
      const LaneCtl* s0c = c0();
      const LaneCtl* s1c = c1();
      if (affine_lane == 0) s0c = h->ctl_mp;
      if (affine_lane == NL - 1 && affine_lane >= 0) s1c = h->ctl_mp;
      if (lead && insum(h) && fuse_upd) {
        // riding steps: beta_1 of the LSQR lanes goes with THIS product's leaders too; a lane without a step of its own has the
        // control block it brings to this product published as it is (ride_leader, kind NONE)
        pend[0] = b0;
        pend[1] = b1;
        pend_xseq = 0;
        if (h->comm) {  // (halo mode: ||rhs||^2 runs over the ranks' owned parts)
          if (int rc = prepare_step(h, pend[0], pend[1], /*sharded=*/true)) return rc;
          pend_xseq = h->last_xseq;
        }
        have_pend = true;
        const StepArgs* pre = pre_args(false);
        if (pend[0].kind == STEP_NONE) pend[0].state = const_cast<LaneCtl*>(s0c);
        if (pend[1].kind == STEP_NONE) pend[1].state = const_cast<LaneCtl*>(s1c);
        launch_spmv<NL>(h, TAG_A, LP, SP, SP, s0c, s1c, h->pS2, seg_none(), seg_none(), false, pre);
        adopt_pend();
      } else {
        if (int rc = launch_step(h, b0.kind ? b0 : b1, b0.kind ? b1 : none, /*sharded=*/h->halo)) return rc;
        launch_spmv<NL>(h, TAG_A, LP, SP, SP, s0c, s1c, h->pS2);
      }
      StepArgs s0 = none, s1 = none;
      UpdSeg w0 = seg_none(), w1 = seg_none();
      for (int l = 0; l < NL; ++l) {
        Lane& L = lanes[l];
        if (L.kind != LANE_LSQR) continue;
        (s0.kind ? s1 : s0) = step_args(STEP_LSQR_BEGIN2, L, 0, h->pS2 + (size_t)l * h->strA, nbA, nullptr, 0, prog[l]);
        (w0.nblk ? w1 : w0) = lsqr_winit_seg(l);
      }
      if (fuse_upd && !s1.kind) {
        // the least-norm lane's beta_1 step shares the launch (it un-parks the lane: must follow the start-up product)
        for (int l = 0; l < NL; ++l)
          if (is_ln(lanes[l].kind)) {
            if (l == affine_lane)  // ||rhs||^2 came out of the start-up product
              s1 = step_args(lane_begin_kind(lanes[l]), lanes[l], 0, h->pS2 + (size_t)l * h->strA, nbA, nullptr, 0, prog[l]);
            else
              s1 = step_args(lane_begin_kind(lanes[l]), lanes[l], 0, h->pEm[l], gm, nullptr, 0, prog[l]);
            ln_begun = true;
          }
        // (riding steps: a MINRES lane's beta_1 step -- it un-parks the lane: must follow the start-up product -- pairs up too)
        if (!s1.kind && lead && !h->comm && minres_lane == 1) {
          s1 = step_args(STEP_MINRES_BEGIN, lanes[1], 0, h->pEm[1], gm, nullptr, 0, prog[1]);
          minres_begun = true;
        }
      }
      if (affine_lane >= 0) {  // keep A z - shift = -rhs before the first A product overwrites the lane
        UpdSeg u = seg_none();
        u.kind = UPD_NEG_COPY;
        u.src = SP;
        u.lane = affine_lane;
        u.nblk = gm;
        u.a = lanes[affine_lane].affine_out;
        u.len = m;
        (w0.nblk ? w1 : w0) = u;
      }
      // (riding steps: alpha_1 / the least-norm lane's beta_1 go with the first A' product of the loop)
      if (lead) {
        if (int rc = post_step(s0, s1, /*sharded=*/true)) return rc;
      } else {
        if (int rc = launch_step(h, s0, s1, /*sharded=*/true)) return rc;
      }
      if (fuse_upd) {  // w_1 rides in the first A' product
        winit[0] = w0;
        winit[1] = w1;
      } else {
        launch_updates<NL>(h, w0, w1, seg_none());
      }
    }
    for (int l = 0; l < NL; ++l)
      if (is_ln(lanes[l].kind) && !ln_begun)
        if (int rc = launch_step(h, step_args(lane_begin_kind(lanes[l]), lanes[l], 0, h->pEm[l], gm, nullptr, 0, prog[l]), none,
                                 /*sharded=*/true))
          return rc;
    if (minres_lane >= 0 && !minres_begun)  // (un-parks the lane: must follow the LSQR lane's start-up product)
      if (int rc = launch_step(h, step_args(STEP_MINRES_BEGIN, lanes[minres_lane], 0, h->pEm[minres_lane], gm, nullptr, 0,
                                            prog[minres_lane]),
                               none, /*sharded=*/true))
        return rc;
    return 0;
  }

  // ------------------------------------------------------------------ one joint iteration
  // A MINRES lane (solve_two_extras) shares the two products of an iteration with the other recurrence: tmp = A' r2
  // rides in the A' product, q = (A tmp + lambda r2) / beta in the A product; then its element-wise stages E1 -> scalar
  // step A -> E2 -> step B.  Stage E3 (w, x) only needs the scalars of step B: it rides in the A' product of the NEXT
  // iteration and its stopping tests (step C) share the step launch that follows that product -- one short
  // element-wise launch and one scalar launch more per iteration than the other recurrence alone.
  //
  // first half-step of every lane: the A' product (LSQR's update of the previous iteration and MINRES' stage E3 riding), its steps
  int half_step_at() {
    lu[0] = lu[1] = seg_none();
    nlu = 0;
    if (it > 1) {
      for (int l = 0; l < NL; ++l)
        if (lanes[l].kind == LANE_LSQR) lu[nlu++] = lsqr_upd_seg(l, it - 1);
    } else {
      lu[0] = winit[0];  // fused runs: w_1 = v_1 (empty segments otherwise)
      lu[1] = winit[1];
    }
    // MINRES: stage E3 of the PREVIOUS iteration (w, x and ||x||^2 for its stopping tests)
    if (minres_lane >= 0 && it > 1) {
      const UpdSeg e3 = minres_seg(3, it - 1, SPcur);
      if (fuse_upd) lu[nlu < 2 ? nlu : 1] = e3;
      else launch_updates<NL>(h, e3, seg_none(), seg_none());
    }
    int npT = 0;
    if (fuse_upd) {
      const StepArgs* pre = pre_args(true);
      if (int rc = at_product<NL>(h, SPcur, LP, t0(), t1(), h->pS, &npT, lu[0], lu[1], pre)) return rc;
      if (pre) adopt_pend();
    } else {
      if (int rc = at_product<NL>(h, SPcur, LP, t0(), t1(), h->pS, &npT)) return rc;
    }
    StepArgs sa[2] = {none, none};
    for (int l = 0; l < NL; ++l) sa[l] = step_after_at(l, npT);
    // sums over n-vectors: replicated (no all-reduce) unless the n-vectors are column windows (halo mode); MINRES' sums
    // run over (row-sharded) m-vectors
    const bool sh0 = lanes[0].kind == LANE_MINRES ? true : h->halo;
    const bool sh1 = lanes[NL - 1].kind == LANE_MINRES ? true : h->halo;
    if (!h->comm) return post_step(sa[0], NL == 2 ? sa[1] : none, false);
    if (lead && sh0 && sh1) return post_step(sa[0], sa[1], true);  // (halo mode, LSQR / CRAIG lanes: both steps sum gathered n-sums)
    if (NL == 2 && split_steps && sh0 != sh1) {
      if (int rc = launch_step(h, sa[0], none, sh0)) return rc;
      return launch_step(h, sa[1], none, sh1);
    }
    if (NL == 2) return launch_step(h, sa[0].kind ? sa[0] : sa[1], sa[0].kind ? sa[1] : none, sa[0].kind ? sh0 : sh1, sa[0].kind ? sh1 : 0);
    if (sa[0].kind) return launch_step(h, sa[0], none, sh0);
    return 0;
  }
  // second half-step: the A product (the least-norm lane's updates of this iteration riding), its steps, MINRES' stages
  int half_step_a() {
    UpdSeg cu[2] = {seg_none(), seg_none()};
    for (int l = 0; l < NL; ++l)
      if (is_ln(lanes[l].kind)) ln_upd_segs(l, cu[0], cu[1]);
    if (fuse_upd) {
      const StepArgs* pre = pre_args(false);
      launch_spmv<NL>(h, TAG_A, LP, SPcur, SPalt, c0(), c1(), h->pS2, cu[0], cu[1], false, pre);
      pa_last = h->pS2;
      if (pre) adopt_pend();
      std::swap(SPcur, SPalt);
    } else {
      // (at most three segments: lanes <= 2 and only one of them can be CRAIG)
      if (nlu == 2) launch_updates<NL>(h, lu[0], lu[1], seg_none());
      else launch_updates<NL>(h, lu[0], cu[0], cu[1]);
      launch_spmv<NL>(h, TAG_A, LP, SPcur, SPcur, c0(), c1(), h->pS2);
      pa_last = h->pS2;
    }
    // A MINRES lane the host has SEEN finished (a zero right-hand side -- hprod! Val(1) on a model without curvature in the
    // constraints --, or an early convergence): its stand-alone launches would exit at once, ~3.5 us each; skipped.  One GPU
    // only: sharded, every rank would have to see it at the same iteration.  (Its riding / shared steps stay: they cost nothing.)
    const bool mdead = minres_lane >= 0 && !h->comm && load_progress(&h->prog_host[minres_lane]).done;
    // MINRES: E1 on q (now in the current pair's lane) before its scalar step A -- with riding steps on one GPU, E1, the step
    // and E2 are ONE launch (k_minres_mid: every workgroup does E1, waits for the leader's record, does E2 on the same elements)
    // (every workgroup of that launch must be resident at once -- the waiting ones hold their slots: the grid has to fit the
    // device with a margin for whatever else runs; should another kernel take the slots all the same, the bounded waits end the
    // call, ride_failed() switches the merge off and the call is repeated on three launches)
    const bool mmid = minres_lane >= 0 && !mdead && lead && NL == 2 && !h->comm && h->minres_merge && h->mm_ptag != nullptr &&
                      4 * (1 + gm) <= 3 * h->mmid_cap;
    if (minres_lane >= 0 && !mdead && !mmid) launch_updates<NL>(h, minres_seg(1, it, SPcur), seg_none(), seg_none());
    StepArgs sb[2] = {none, none};
    for (int l = 0; l < NL; ++l) sb[l] = step_after_a(l);
    if (minres_lane >= 0 && lead && NL == 2) {
      // MINRES' step A must run before E2; the other lane's step is only needed by the NEXT A' launch (its epilogue and its
      // riding update) and waits for MINRES' step B to ride there with it
      if (mmid) {
        const UpdSeg e1 = minres_seg(1, it, SPcur), e2 = minres_seg(2, it, SPcur);
        hipLaunchKernelGGL(k_minres_mid, dim3(1 + e1.nblk), dim3(kBlock), 0, s, e1, e2, sb[minres_lane], h->mm_ptag, h->ride_rec2,
                           (unsigned int)++h->ride_seq, reinterpret_cast<unsigned long long*>(h->hscal_dev + 15));
        h->launches++;
        h->mmid_launches++;
      } else if (!mdead) {
        if (int rc = launch_step(h, sb[minres_lane], none, /*sharded=*/true)) return rc;
        launch_updates<NL>(h, minres_seg(2, it, SPcur), seg_none(), seg_none());
      }
      StepArgs pair[2];
      pair[minres_lane] = minres_step(STEP_MINRES_B, it);
      pair[1 - minres_lane] = sb[1 - minres_lane];
      return post_step(pair[0], pair[1], true);
    }
    if (!h->comm || lead) {
      if (int rc = post_step(sb[0], NL == 2 ? sb[1] : none, true)) return rc;
    } else {
      if (int rc = launch_step(h, sb[0], sb[1], /*sharded=*/true)) return rc;
    }
    if (minres_lane >= 0 && !mdead) {  // E2 -> scalar step B (beta, the rotation, the coefficients of E3 and of the next products)
      launch_updates<NL>(h, minres_seg(2, it, SPcur), seg_none(), seg_none());
      if (int rc = launch_step(h, minres_step(STEP_MINRES_B, it), none, /*sharded=*/true)) return rc;
    }
    return 0;
  }

  // One launch for both half-steps (k_iter_fused): the A' product with what rides in it, the steps behind it (mid leaders), the A
  // product with what rides in it.  Needs the previous product's steps pending (they are the head leaders' work).
  int iteration_fused() {
    lu[0] = lu[1] = seg_none();
    nlu = 0;
    if (it > 1) {
      for (int l = 0; l < NL; ++l)
        if (lanes[l].kind == LANE_LSQR) lu[nlu++] = lsqr_upd_seg(l, it - 1);
    } else {
      lu[0] = winit[0];
      lu[1] = winit[1];
    }
    const StepArgs* pre = pre_args(true);
    StepArgs sh[2] = {pre[0], pre[NL - 1]}, sm[2];
    // halo-sharded with rows shared with the neighbours: the exchange and the finish of the overlap rows ride in this launch
    // (fuse_halo_wg); the finish workgroups' partials follow the blocks'
    // (the HALO kernel also whenever the leaders exchange -- its leaders have the exchange compiled in; no shared rows: no halo workgroups)
    const bool shared_rows = h->comm && h->halo && h->ovl + h->ovr > 0;
    const bool with_halo = shared_rows || (h->comm && h->halo && insum_table(h) != nullptr);
    FuseHalo fh{};
    HaloRows hr{};
    if (with_halo && !shared_rows) hr = HaloRows{0, h->n, h->halo_raw};
    if (shared_rows) {
      const int64_t t = h->ovl + h->ovr;
      double* rl = h->halo_recv + (size_t)(h->halo_calls++ & 1) * (size_t)t * 2;
      if (!h->comm->halo_fused_args(rl, h->ovl, h->ovr, fh)) {
        h->err = "internal: one-launch iteration on a communicator without in-launch halo exchange";
        return FPSQ_ERR_STATE;
      }
      fh.raw = h->halo_raw;
      fh.recv = rl;
      fh.tl = h->ovl;
      fh.tr = h->ovr;
      fh.tail0 = h->n - h->ovr;
      fh.gf = h->halo_gf;
      fh.nwg = (2 * kHaloCopy + h->halo_gf + 7) / 8 * 8;
      fh.depL = h->fz_depL;
      fh.depR = h->fz_depR;
      hr = HaloRows{h->ovl, h->n - h->ovr, h->halo_raw};
    }
    for (int l = 0; l < NL; ++l) {
      sm[l] = step_after_at(l, h->AT.nblk + (shared_rows ? h->halo_gf : 0));
      sm[l].state = sh[l].state_out;  // (what the head step leaves: the mid leaders recompute it, nobody reads this pointer)
      sm[l].state_out = lanes[l].state_alt2;
      sm[l].prod_ctl_off = 0;
    }
    uint32_t mid_xseq = 0;
    if (h->comm) {  // (halo mode: the mid leaders' sums run over the ranks -- the exchange behind the head steps')
      if (int rc = prepare_step(h, sm[0], sm[1], true)) return rc;
      mid_xseq = h->last_xseq;
    }
    UpdSeg cu[2] = {seg_none(), seg_none()};
    for (int l = 0; l < NL; ++l)
      if (is_ln(lanes[l].kind)) ln_upd_segs(l, cu[0], cu[1]);
    FuseGrid fg{};
    fg.bpx = (h->AT.nblk + 7) / 8;
    {
      const int R = h->resident_wgs - kRideCand;
      const int n2 = !h->atl_two || h->AT.nblk <= R ? 0 : std::min(R, h->AT.nblk - R);
      const int n2e = std::min(n2 / 8, fg.bpx / 2);
      fg.n2 = 8 * n2e;
      fg.nwg_t = 8 * (fg.bpx - n2e);
    }
    fg.nupd_t = (lu[0].nblk + lu[1].nblk + 7) / 8 * 8;
    fg.gpx = (h->RA.view.ng + 7) / 8;
    fg.rot = h->fuse_rotate;
    RideArgs ra{}, rb{};
    ra.rec = h->ride_rec;
    ra.want = (unsigned int)++h->ride_seq;
    ra.pub = ra.want;
    ra.err = reinterpret_cast<unsigned long long*>(h->hscal_dev + 15);
    ra.delay = h->ride_delay;
    rb = ra;
    rb.rec = h->ride_rec2;
    rb.delay = h->ride_delay_mid;
    ra.xseq = h->ride_xseq;  // (pre_args: the pending head steps' exchange)
    ra.xt = ra.xseq ? insum_table(h) : nullptr;
    rb.xseq = mid_xseq;
    rb.xt = mid_xseq ? insum_table(h) : nullptr;
    // (leaders that wait for a late peer keep everything behind them waiting: blocks, row groups, the other leader set, updates)
    const int more = ra.xt || rb.xt ? h->comm->wait_more() : 0;
    ra.more = rb.more = more;
    FuseArgs fz{};
    fz.more = more;
    fz.blkflag = h->fz_flag;
    fz.ptag = h->fz_ptag;
    fz.dep = h->fz_dep;
    fz.dep2 = shared_rows ? h->fz_dep2 : nullptr;
    fz.want = ra.want;
    fz.pub = h->fuse_break ? ~ra.want : ra.want;
    fz.err = ra.err;
    double* part_a = pa_last == h->pS2 ? h->pS2b : h->pS2;  // (not the array this launch's leaders read)
    const dim3 grid(kRideCand + fg.nwg_t + fh.nwg + kRideCand + fg.nupd_t + 8 * fg.gpx + cu[0].nblk + cu[1].nblk);
    if (h->fuse_probe_at > 0 && h->fused_total + 1 == h->fuse_probe_at) {  // developer probe: this launch leaves time stamps
      h->fuse_probe_grid = (int)grid.x;
      h->fuse_probe_layout = {kRideCand, fg.nwg_t + fh.nwg, kRideCand, 8 * fg.gpx, fg.nupd_t, cu[0].nblk + cu[1].nblk};
      if (dalloc(h, &h->fuse_probe_buf, (size_t)grid.x * 4) == 0) {
        hipMemsetAsync(h->fuse_probe_buf, 0, (size_t)grid.x * 32, h->stream);
        fz.dbg = h->fuse_probe_buf;
      }
    }
    h->fused_total++;
#define FPSQ_LAUNCH_FUSED(...)                                                                                                        \
    launch_product(h, k_iter_fused<__VA_ARGS__>, grid, h->AT.view(), h->RA.view, (const double*)SPcur, LP, SPalt, part_a, h->strA, fg, \
                   lu[0], lu[1], cu[0], cu[1], sh[0], sh[1], sm[0], sm[1], ra, rb, fz, hr, fh)
    if (h->AT.sorted && with_halo) FPSQ_LAUNCH_FUSED(true, true);
    else if (h->AT.sorted) FPSQ_LAUNCH_FUSED(true, false);
    else if (with_halo) FPSQ_LAUNCH_FUSED(false, true);
    else FPSQ_LAUNCH_FUSED(false, false);
#undef FPSQ_LAUNCH_FUSED
    h->launches++;
    h->spmv_launches++;
    h->prod_a[1]++;
    h->prod_at[1]++;
    h->fused_launches++;
    pa_last = part_a;
    // the lanes live in their third copies now; the other two are free for the next launch's two steps
    for (int l = 0; l < NL; ++l) {
      Lane& L = lanes[l];
      void* s0 = L.state;
      L.state = L.state_alt2;
      L.state_alt2 = L.state_alt;
      L.state_alt = s0;
      L.ctl = reinterpret_cast<LaneCtl*>(L.state);
      L.ctlT = L.ctl;
    }
    have_pend = false;
    std::swap(SPcur, SPalt);
    StepArgs sb[2] = {none, none};
    for (int l = 0; l < NL; ++l) sb[l] = step_after_a(l);
    return post_step(sb[0], sb[1], true);
  }

  // K joint iterations in ONE launch (k_iter_multi, fpsq_multi.hip.h): iterations it .. it + K - 1.  Needs what iteration_fused
  // needs (the previous product's steps pending) and it >= 2 (iteration 1 carries the start-up's w_1 segments).
  int iteration_multi(int K) {
    MultiArgs M{};
    M.K = K;
    M.it0 = (int32_t)it;
    const StepArgs* pre = pre_args(true);
    int nut = 0;
    for (int l = 0; l < NL; ++l) {
      M.sh[l] = pre[l];
      M.sm[l] = step_after_at(l, h->AT.nblk);
      M.sm[l].state = nullptr;
      M.sm[l].state_out = nullptr;
      M.sm[l].prod_ctl_off = 0;
      M.commit[l][0] = lanes[l].state_alt;
      M.commit[l][1] = lanes[l].state_alt2;
      M.pw[l][0] = h->pW[l];
      M.pw[l][1] = h->pWalt[l];
      M.p1seg[l] = 3;
      if (lanes[l].kind == LANE_LSQR) {
        M.p1seg[l] = nut;
        M.ut[nut++] = lsqr_upd_seg(l, it - 1);
      }
    }
    for (int k = nut; k < 2; ++k) M.ut[k] = seg_none();
    M.ua[0] = M.ua[1] = seg_none();
    for (int l = 0; l < NL; ++l)
      if (is_ln(lanes[l].kind)) ln_upd_segs(l, M.ua[0], M.ua[1]);
    M.n1 = gm;
    FuseGrid& fg = M.fg;
    fg.bpx = (h->AT.nblk + 7) / 8;
    {
      const int R = h->resident_wgs - kRideCand;
      const int n2 = !h->atl_two || h->AT.nblk <= R ? 0 : std::min(R, h->AT.nblk - R);
      const int n2e = std::min(n2 / 8, fg.bpx / 2);
      fg.n2 = 8 * n2e;
      fg.nwg_t = 8 * (fg.bpx - n2e);
    }
    // (few real update workgroups, each walking several virtual ones: see k_iter_multi)
    fg.nupd_t = std::min((M.ut[0].nblk + M.ut[1].nblk + 7) / 8 * 8, h->multi_upd_t);
    fg.gpx = (h->RA.view.ng + 7) / 8;
    fg.rot = h->fuse_rotate;
    // CRAIG's long update one iteration later, behind the next A' blocks (FPSQ_MULTI_DEFER_LONG=0: with the short one)
    M.nlong = h->multi_defer_long ? (M.ua[0].nblk + 7) / 8 * 8 : 0;
    M.nupd_a = std::min(((M.nlong ? 0 : M.ua[0].nblk) + M.ua[1].nblk + 7) / 8 * 8, h->multi_upd_a);
    M.per_iter = kRideCand + fg.nwg_t + M.nlong + kRideCand + 8 * fg.gpx + fg.nupd_t + M.nupd_a;
    M.seq0 = (uint32_t)(h->ride_seq + 1);
    h->ride_seq += (unsigned long long)K;
    M.sp[0] = SPcur;
    M.sp[1] = SPalt;
    M.sp0 = 0;
    M.lp[0] = LP;
    M.lp[1] = LPalt;
    M.lp0 = 0;
    M.part_last = pa_last == h->pS2 ? h->pS2b : h->pS2;  // (not the array this launch's first leaders read)
    M.pstride_a = h->strA;
    M.rec_h = h->mz_rec_h;
    M.rec_m = h->mz_rec_m;
    M.srec = h->mz_srec;
    M.flag[0] = h->fz_flag;
    M.flag[1] = h->mz_flag2;
    M.ptag[0] = h->fz_ptag;
    M.ptag[1] = h->mz_ptag2;
    for (int q = 0; q < 2; ++q) {
      M.gflag[q] = h->mz_gflag[q];
      M.atag[q] = h->mz_atag[q];
      M.utag[q] = h->mz_utag[q];
    }
    M.dep = h->fz_dep;
    M.bdep = h->mz_bdep;
    M.hdone = h->mz_hdone;
    M.err = reinterpret_cast<unsigned long long*>(h->hscal_dev + 15);
    M.delay_h = h->ride_delay;
    M.delay_m = h->ride_delay_mid;
    M.break_pub = h->fuse_break ? ~0u : 0u;
    const dim3 grid((unsigned)M.per_iter * (unsigned)K + (unsigned)M.nlong);
    if (h->AT.sorted) launch_product(h, k_iter_multi<true>, grid, h->AT.view(), h->RA.view, M);
    else launch_product(h, k_iter_multi<false>, grid, h->AT.view(), h->RA.view, M);
    h->launches++;
    h->spmv_launches++;
    h->prod_a[1] += K;
    h->prod_at[1] += K;
    h->fused_launches += K;
    h->fused_total += K;
    h->multi_launches++;
    h->multi_iters += K;
    pa_last = M.part_last;
    // the lanes live where the last iteration's mid leaders committed; the other two copies are free for the next launch
    for (int l = 0; l < NL; ++l) {
      Lane& L = lanes[l];
      void* cur = L.state;
      void* fin = M.commit[l][(K - 1) & 1];
      void* oth = M.commit[l][K & 1];
      L.state = fin;
      L.state_alt = cur;
      L.state_alt2 = oth;
      L.ctl = reinterpret_cast<LaneCtl*>(L.state);
      L.ctlT = L.ctl;
    }
    have_pend = false;
    if (K & 1) {
      std::swap(SPcur, SPalt);
      std::swap(LP, LPalt);
    }
    it += K - 1;  // (run() counted the first one)
    StepArgs sb[2] = {none, none};
    for (int l = 0; l < NL; ++l) sb[l] = step_after_a(l);
    return post_step(sb[0], sb[1], true);
  }

  // ------------------------------------------------------------------ the host's pacing
  // the gated final LSQR flush + the caller's epilogue behind iteration `it` (see the comment above)
  int enqueue_speculative() {
    if (tail == nullptr || !fuse_upd) return 0;
    UpdSeg seg[2] = {seg_none(), seg_none()};
    int ns = 0;
    for (int l = 0; l < NL; ++l)
      if (lanes[l].kind == LANE_LSQR) {
        seg[ns] = lsqr_upd_seg(l, it);
        seg[ns++].gate = lanes[NL - 1 - l].ctl;  // the other lane of the call (NL = 1: itself)
      }
    TailCtx t;
    t.gates = Gates{lanes[0].ctl, lanes[NL - 1].ctl};
    if (req.absorb_flush && ns == 1) t.flush = seg[0];  // applied by the tail's first kernel (k_ys)
    else launch_updates<NL>(h, seg[0], seg[1], seg_none());
    const int64_t l0 = h->launches;
    const int rc = (*tail)(t);
    tail_launches += h->launches - l0;  // (the caller's epilogue, not the loop: fpsq_info.last_loop_launches)
    if (rc) return rc;
    spec_it = it;
    return 0;
  }
  // the host waits until every unfinished lane has reported iteration `target` (minus its lag) or has ended
  int wait_lanes(int64_t target) {
    for (int l = 0; l < NL; ++l) {
      if (load_progress(&h->prog_host[l]).done) continue;
      const int32_t* ddone = &lanes[l].ctl->done;
      if (int rc = wait_progress(h, l, (int)target - lane_lag(lanes[l]), ddone, lane_iter_ptr(lanes[l]))) return rc;
    }
    return 0;
  }
  // Sharded: every rank must enqueue the same collectives: decide at fixed iteration boundaries from the (replicated,
  // bitwise identical) device state, never from the timing of the progress word.  With the iteration count of the
  // previous call known (halo mode; the same on every rank) the first look is AT that count, with the gated flush
  // and epilogue already enqueued behind it: a repeating count costs no stream synchronisation inside the loop.
  int pace_sharded(bool& stop) {
    bool boundary = it == itmax_all;
    if (expect > 0) {
      if (it == expect) {
        if (int rc = flush_pend(true)) return rc;  // (the gated kernels must see this iteration's verdict)
        if (int rc = enqueue_speculative()) return rc;
        boundary = true;
      } else if (it > expect && (it - expect) % look == 0) {
        boundary = true;
      }
    } else if (it % look == 0) {
      boundary = true;
    }
    if (boundary) {
      if (int rc = flush_pend(true)) return rc;  // (so must the host; the same launches on every rank)
      HIPCHK(h, hipStreamSynchronize(s));
      if (h->comm->failed()) {  // (peer-to-peer route: a peer's record never came; nothing later in this call can be right)
        h->info.p2p_timeouts++;
        h->err = "peer-to-peer exchange: a peer's record did not arrive (bounded wait expired)";
        return FPSQ_ERR_TIMEOUT;
      }
      if (all_done()) stop = true;
    }
    return 0;
  }
  int pace_single(bool& stop) {
    if (all_done()) {
      stop = true;
      return 0;
    }
    if (*reinterpret_cast<volatile uint64_t*>(h->hscal + 15) != 0) {  // (an expired wait inside a launch: see wait_progress)
      stop = true;
      return 0;  // (call_end reports it -- and switches the handle to two launches per iteration: ride_failed)
    }
    // before the expected count the steps publish nothing (but the end of a recurrence): enqueue on
    if (it < expect) return 0;
    // bound the run-ahead of the host on the slowest unfinished lane
    int slow = INT32_MAX;
    for (int l = 0; l < NL; ++l) {
      const Progress ps = load_progress(&h->prog_host[l]);
      if (!ps.done) slow = std::min(slow, (int)ps.iter + lane_lag(lanes[l]));
    }
    if (it > expect && it - slow >= look) {
      if (int rc = flush_pend(true)) return rc;  // (the host is about to wait for the pending steps' progress)
      if (int rc = wait_lanes(it - look + 1)) return rc;
      if (all_done()) {
        stop = true;
        return 0;
      }
    }
    // Consecutive calls of one kind (the evaluations of a line search, the CG steps of a Newton iteration) mostly take
    // the same number of iterations: do not enqueue iteration expect + 1 before the device has finished iteration
    // `expect`.  When the count repeats, no launch is enqueued past convergence (each costs ~3.5 us of GPU time even
    // though it exits at once: ~50 us per evaluation at lookahead 4); when it does not, this is one short bubble.
    if (expect > 0 && it == expect) {
      if (int rc = flush_pend(true)) return rc;  // (the gated kernels and the host must see this iteration's verdict)
      if (int rc = enqueue_speculative()) return rc;
      if (int rc = wait_lanes(it)) return rc;
      if (all_done()) stop = true;
    }
    return 0;
  }

  // ------------------------------------------------------------------ behind the loop
  int finish() {
    if (!h->comm && !all_done()) {
      // The loop ran out of iterations (itmax) before the host saw every lane end.  The steps still in the stream will publish
      // those ends into the progress words -- which the NEXT run of this call (the second lane of an unfused call, the extras
      // lanes of hprod! Val(1)) resets on the host and then polls: a late "done" of THIS run would make it stop enqueueing at
      // once and leave its recurrence unfinished (found by the fixed-iteration tests: statistics of the second lane all zero).
      // Drain the stream, so that every word says what this run ended with.  (Only the itmax exit comes here: the other exits
      // of the loop have seen `done`; a sharded run has synchronised at this boundary already.)
      if (int rc = flush_pend(true)) return rc;
      HIPCHK(h, hipStreamSynchronize(s));
    }
    if (all_done()) {  // the iteration at which the last recurrence finished (its progress word says so)
      int64_t e = 0;
      for (int l = 0; l < NL; ++l) e = std::max<int64_t>(e, h->prog_host[l].iter + lane_lag(lanes[l]));
      expect_slot[1] = expect_slot[0];
      expect_slot[0] = e;
    }
    if (int rc = flush_pend(true)) return rc;
    ht_mark(h, 4);
    if (spec_it >= 0 && spec_it == it && all_done()) {
      // every recurrence ended at or before the iteration the speculative flush + tail were enqueued behind: their gates
      // were open, the call's epilogue is already in the stream
      res.tail_was_run = true;
      return 0;
    }
    // the last LSQR update (iteration `it`) has not been enqueued yet
    UpdSeg seg[2] = {seg_none(), seg_none()};
    int ns = 0;
    for (int l = 0; l < NL; ++l)
      if (lanes[l].kind == LANE_LSQR && it >= 1) seg[ns++] = lsqr_upd_seg(l, it);
    if (it == 0) {  // no iteration ran (itmax = 0): the pending w_1 / x = 0 start-up still has to happen
      seg[0] = winit[0];
      seg[1] = winit[1];
    }
    // MINRES: stage E3 and the stopping tests of the last enqueued iteration (no-ops when it ended earlier)
    if (req.absorb_flush && tail != nullptr && ns == 1 && it >= 1 && minres_lane < 0)
      res.flush = seg[0];  // the caller's epilogue starts with k_ys, which applies it
    else
      launch_updates<NL>(h, seg[0], seg[1], minres_lane >= 0 && it >= 1 ? minres_seg(3, it, SPcur) : seg_none());
    if (minres_lane >= 0 && it >= 1)
      if (int rc = launch_step(h, minres_step(STEP_MINRES_C, it), none, /*sharded=*/true)) return rc;
    return 0;  // the final stats were left in lanes[l].st by the step that ended each recurrence
  }

  int run() {
    setup();
    if (int rc = startup()) return rc;
    const int64_t launches0 = h->launches;
    while (it < itmax_all) {
      ++it;
      // several iterations per launch while the expected count (or itmax) leaves room for at least two; never across the count:
      // the gated flush and the epilogue go right behind it
      int K = 1;
      if (can_multi && have_pend && it >= 2 && expect > 0 && it <= expect)
        K = (int)std::min<int64_t>(std::min<int64_t>(h->multi_max, expect - it + 1), itmax_all - it + 1);
      if (K >= 2) {
        if (int rc = iteration_multi(K)) return rc;
      } else if (can_fuse && have_pend) {
        if (int rc = iteration_fused()) return rc;
      } else {
        if (int rc = half_step_at()) return rc;
        if (int rc = half_step_a()) return rc;
      }
      bool stop = false;
      if (int rc = h->comm ? pace_sharded(stop) : pace_single(stop)) return rc;
      if (stop) break;
    }
    h->loop_iters += it;
    h->loop_launches += h->launches - launches0 - tail_launches;
    return finish();
  }
};

template <int NL>
int run_krylov(fpsq_handle h, Lane* lanes, const TailFn* tail, const RunRequest& req, RunResult* res) {
  KrylovRun<NL> r(h, lanes, tail, req);
  const int rc = r.run();
  if (res) *res = r.res;
  return rc;
}

// (one recurrence after the other: the first run serves the request, and the caller runs its epilogue behind them)
int run_lanes(fpsq_handle h, Lane* lanes, int nlanes, const TailFn* tail = nullptr, const RunRequest& req = {},
              RunResult* res = nullptr) {
  if (nlanes == 2 && h->opt.fuse_two_rhs) return run_krylov<2>(h, lanes, (!h->comm || h->halo) ? tail : nullptr, req, res);
  for (int l = 0; l < nlanes; ++l)
    if (int rc = run_krylov<1>(h, lanes + l, nullptr, l == 0 ? req : RunRequest{}, nullptr)) return rc;
  return 0;
}

}  // namespace
