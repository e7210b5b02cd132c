// fpsq.hip -- host side of libfpsq.so's iterative path: the C ABI of include/fpsq.h and the scaffolding of its calls (stream
// adoption, call_begin / call_end, the solves that combine Krylov lanes).  ONE translation unit, cut into headers included below
// in the order of the text: fpsq_handle.hip.h (the handle and its create-time switches; fpsq_comm.hip.h: the communicators),
// fpsq_structure.hip.h (Jacobian storage: uploads of the layouts of A and A'), fpsq_launch.hip.h (product launches),
// fpsq_run.hip.h (the stream orchestration of the device-resident Krylov recurrences).
//
// Reference path replaced: src/solve_linear_system.jl:45-140 + src/solve_two_systems_struct.jl:167-244
// (FletcherPenaltySolver.jl v0.3.0), whose arithmetic runs in Krylov.jl on the CPU.
#include "../../include/fpsq.h"
#include "fpsq_spmv.hip.h"
#include "fpsq_multi.hip.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>  // types only; the library is dlopen'ed on first use

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

using namespace fpsq;

namespace {

thread_local std::string g_create_error;

}  // namespace

// the rest of this translation unit, in this order (each header includes the ones before it)
#include "fpsq_handle.hip.h"     // DevCsr, DevRgcs, [fpsq_comm.hip.h: the communicators], fpsq_solver_s, dalloc
#include "fpsq_structure.hip.h"  // uploads of the layouts, workspaces, finish_structure
#include "fpsq_launch.hip.h"     // product launches, halo_finish, wait_progress
#include "fpsq_run.hip.h"        // KrylovRun<NL>, run_krylov, run_lanes
#include "fpsq_qp_csr.hip.h"     // k_qp_csr<LG, MODE>: the products with R of a sparse objective Hessian
#include "fpsq_qcsr.h"           // the host-side check and split Q = diag(q) + R

namespace {

// Halo mode, once, at the first (collective) solve call: the padded counts of the gather segment = the maxima over
// the ranks of the local partial counts, then the segment itself (see fpsq_solver_s::seg).
int ensure_gather_layout(fpsq_handle h) {
  if (!h->comm || !h->halo || h->gather_ready) return 0;
  const int P = h->comm->nranks;
  const int gn = ew_grid(h->n), gm = ew_grid(h->m);
  const double mine[4] = {(double)gn, (double)(h->AT.nblk + h->halo_gf), (double)npart_A(h), (double)gm};
  double* dsend = h->dscal;      // 4 doubles
  double* drecv = nullptr;       // 4 P doubles
  if (int rc = dalloc(h, &drecv, (size_t)4 * P)) return rc;
  HIPCHK(h, hipMemcpyAsync(dsend, mine, sizeof mine, hipMemcpyHostToDevice, h->stream));
  if (int rc = h->comm->allgather(dsend, drecv, 4, h->stream)) {
    h->err = h->comm->err;
    return rc;
  }
  std::vector<double> all((size_t)4 * P);
  HIPCHK(h, hipMemcpyAsync(all.data(), drecv, all.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dfree(h, &drecv);
  int c[4] = {0, 0, 0, 0};
  for (int r = 0; r < P; ++r)
    for (int k = 0; k < 4; ++k) c[k] = std::max(c[k], (int)all[(size_t)4 * r + k]);
  h->cE = c[0];
  h->cT = c[1];
  h->cA = c[2];
  h->cW = c[3];
  h->seg_len = 2 * (int64_t)h->cE + 2 * (int64_t)h->cT + 2 * (int64_t)h->cA + 7 * (int64_t)h->cW;
  if (int rc = dalloc(h, &h->seg, (size_t)h->seg_len)) return rc;
  if (int rc = dalloc(h, &h->gath, (size_t)h->seg_len * P * 2)) return rc;
  HIPCHK(h, hipMemsetAsync(h->seg, 0, (size_t)h->seg_len * 8, h->stream));  // the padding entries stay zero for good
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double* q = h->seg;
  h->pE = q;
  q += h->cE;
  h->pE2 = q;
  q += h->cE;
  h->pEm[0] = q;
  q += h->cW;
  h->pEm[1] = q;
  q += h->cW;
  h->pS = q;
  h->strT = h->cT;
  q += 2 * h->cT;
  h->pWalt[0] = q;
  q += h->cW;
  h->pWalt[1] = q;
  q += h->cW;
  h->pS2 = q;
  h->strA = h->cA;
  q += 2 * h->cA;
  h->pW[0] = q;
  q += h->cW;
  h->pW[1] = q;
  q += h->cW;
  h->pE3 = q;
  {
    Comm::Buffers B{};
    B.gath[0] = h->gath;
    B.gath[1] = h->gath + (size_t)h->seg_len * P;
    B.halo_recv = h->halo_recv;
    B.ovl = h->ovl;
    B.ovr = h->ovr;
    if (int rc = h->comm->arm(B, h->stream)) {
      h->err = h->comm->err;
      return rc;
    }
  }
  h->gather_ready = true;
  h->info.comm_route = h->comm->route();
  h->info.comm_in_launch_sums = insum(h) ? 1 : 0;
  return 0;
}

int check_ready(fpsq_handle h) {
  if (!h) return FPSQ_ERR_ARG;
  if (!h->have_structure || !h->have_values) {
    h->err = "Jacobian structure/values not set";
    return FPSQ_ERR_STATE;
  }
  hipSetDevice(h->opt.device);
  return ensure_gather_layout(h);
}

// Device-resident arguments are produced on the caller's stream: everything queued there so far must be complete
// before the first kernel / copy of this call touches them (include/fpsq.h, "INPUT READINESS").
// back to the handle's own stream (see fpsq_set_input_stream)
void unadopt_stream(fpsq_handle h) {
  if (!h->adopted) return;
  hipStreamSynchronize(h->stream);
  h->stream = h->own_stream;
  h->adopted = false;
}
void order_inputs(fpsq_handle h) {
  if (!h->in_stream_on || h->adopted) return;
  hipEventRecord(h->ev_in, h->in_stream);
  hipStreamWaitEvent(h->stream, h->ev_in, 0);
}

void call_begin(fpsq_handle h) {
  h->launches = 0;
  h->spmv_launches = 0;
  h->prod_a[0] = h->prod_a[1] = h->prod_at[0] = h->prod_at[1] = 0;
  h->fused_launches = 0;
  h->mmid_launches = 0;
  h->multi_launches = h->multi_iters = 0;
  h->loop_launches = h->loop_iters = 0;
  h->ev_used = 0;
  // device-side timing of the whole call only when profiling is on: an event record is a marker packet the GPU has to
  // process (a few us each); otherwise last_solve_ms is the host's wall time of the call
  if (h->profile) hipEventRecord(h->ev0, h->stream);
  h->t_call = std::chrono::steady_clock::now();
}

// steps riding with leaders: a workgroup's bounded wait for the leaders' record expired (never observed; see kRidePolls)
bool ride_failed(fpsq_handle h) {
  // (the device stores the INTEGER 1 there -- as a double a denormal, which a host running with flush-to-zero would not see)
  volatile uint64_t* w = reinterpret_cast<volatile uint64_t*>(h->hscal + 15);
  if (*w == 0) return false;
  *w = 0;
  h->info.wait_timeouts++;
  h->err = "a bounded wait inside a product launch expired (the leaders' record did not arrive, or -- one-launch iterations -- a block's "
           "flag / partials did not): FPSQ_FUSE_ITER=0 keeps two launches per iteration, FPSQ_RIDE_LEAD=0 the stand-alone steps";
  // (something else held the device for longer than the bound: this handle goes on with two launches per iteration, whose
  // waits involve the leaders only)
  if (h->fused_launches > 0 && h->fuse_ok) {
    h->fuse_ok = false;
    h->fuse_fell_back = true;  // (the entry point repeats the call once: with_fuse_fallback)
  }
  // the same for a MINRES lane's merged launch (k_minres_mid: every workgroup of its grid must be resident at once): back to
  // three launches, whose workgroups wait for nobody, and the call is repeated
  if (h->mmid_launches > 0 && h->minres_merge) {
    h->minres_merge = false;
    h->fuse_fell_back = true;
  }
  return true;
}

int call_end(fpsq_handle h) {
  if (h->profile) hipEventRecord(h->ev1, h->stream);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->comm && h->comm->failed()) {
    h->info.p2p_timeouts++;
    h->err = "peer-to-peer exchange: a peer's record did not arrive (bounded wait expired)";
    return FPSQ_ERR_TIMEOUT;
  }
  if (ride_failed(h)) return FPSQ_ERR_TIMEOUT;
  float ms = 0.f;
  if (h->profile) hipEventElapsedTime(&ms, h->ev0, h->ev1);
  else ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - h->t_call).count();
  h->info.last_solve_ms = ms;
  h->info.last_kernel_launches = h->launches;
  h->info.last_spmv_launches = h->spmv_launches;
  for (int i = 0; i < 2; ++i) {
    h->info.last_prod_a[i] = h->prod_a[i];
    h->info.last_prod_at[i] = h->prod_at[i];
  }
  h->info.last_fused_launches = h->fused_launches;
  h->info.last_multi_launches = h->multi_launches;
  h->info.last_multi_iterations = h->multi_iters;
  h->info.last_loop_iterations = h->loop_iters;
  h->info.last_loop_launches = h->loop_launches;
  double sp = 0.0;
  for (size_t i = 0; i < h->ev_used; ++i) {
    float t = 0.f;
    hipEventElapsedTime(&t, h->ev_pool[i].a, h->ev_pool[i].b);
    sp += t;
  }
  h->info.last_spmv_ms = sp;
  return 0;
}

// End of a call with stream-ordered outputs: the caller's stream waits (event, no host block) for everything enqueued so
// far; the host only waits until the phi reduction -- which rides in the first kernel of the epilogue's tail -- has stored
// the call's sequence number behind its results (host-mapped memory, release store: the values and, from the earlier
// step kernels, the final statistics are there when the number is).
int call_end_ordered(fpsq_handle h, double seq) {
  if (!h->adopted) {
    HIPCHK(h, hipEventRecord(h->ev_out, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->in_stream, h->ev_out, 0));
  }
  volatile double* flag = h->hscal + 3;
  const auto t0 = std::chrono::steady_clock::now();
  int spins = 0;
  while (*flag != seq) {
    if ((++spins & 255) == 0) {
      const hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess) break;  // everything ran (the mapped store is then visible too; if not, the values below are read after a full drain anyway)
      if (q != hipErrorNotReady) {
        h->err = std::string("stream failed in the epilogue: ") + hipGetErrorString(q);
        return FPSQ_ERR_HIP;
      }
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 120.0) {
        h->err = "timeout waiting for the evaluation's scalar results";
        return FPSQ_ERR_TIMEOUT;
      }
    }
  }
  if (h->comm && h->comm->failed()) {
    h->info.p2p_timeouts++;
    h->err = "peer-to-peer exchange: a peer's record did not arrive (bounded wait expired)";
    return FPSQ_ERR_TIMEOUT;
  }
  if (ride_failed(h)) return FPSQ_ERR_TIMEOUT;
  h->info.last_solve_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - h->t_call).count();
  h->info.last_kernel_launches = h->launches;
  h->info.last_spmv_launches = h->spmv_launches;
  for (int i = 0; i < 2; ++i) {
    h->info.last_prod_a[i] = h->prod_a[i];
    h->info.last_prod_at[i] = h->prod_at[i];
  }
  h->info.last_fused_launches = h->fused_launches;
  h->info.last_multi_launches = h->multi_launches;
  h->info.last_multi_iterations = h->multi_iters;
  h->info.last_loop_iterations = h->loop_iters;
  h->info.last_loop_launches = h->loop_launches;
  h->info.last_spmv_ms = 0.0;
  return 0;
}

// true when p is device memory of the handle's GPU (kernels may then use it in place)
bool on_this_device(fpsq_handle h, const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // plain host memory: not an error
    return false;
  }
  return a.type == hipMemoryTypeDevice && a.device == h->opt.device;
}

int soft_rc(const fpsq_stats st[2]) { return (st[0].solved ? 0 : 1) | (st[1].solved ? 0 : 2); }

__global__ void k_mk_params(MinresState* S, MinresParams P, double kdelta) {
  MinresState* s = S + blockIdx.x;
  minres_set_params(s, P);
  s->kmode = 1;
  s->kdelta = kdelta;
  s->lambda = 0.0;
  s->ctl.skip = 0;
}

// Both systems K [p; q] = [bp_l; bq_l], l = 0, 1, by MINRES on K = [I A'; A -delta I] (order n + m), the two recurrences
// in lock-step on interleaved vectors: per iteration one two-RHS A' product, one two-RHS A product, three element-wise
// stages over n + m and three scalar steps.  Not a path of the reference (its `solve_two_mixed` is LSQR + CRAIG, the
// default here): BASELINE.json's north_star / configs[1] name it ("MINRES matrix-free") and SURVEY 8(b) lists it in the
// method enum.  Tolerances: the reference's MINRES set (ne_atol, ne_rtol, ne_etol, ne_conlim; ne_itmax = 0 -> 2 (n + m)).
// Null right-hand sides are zero.  Solutions to (p0, q0, p1, q1); stats to h->hstats[0 / 1].
int minres_k_device(fpsq_handle h, const double* bp0, const double* bq0, const double* bp1, const double* bq1, double* p0,
                    double* q0, double* p1, double* q1) {
  if (h->comm) {
    h->err = "kkt_method = MINRES_K is single-GPU (use the default LSQR + CRAIG method on a sharded handle)";
    return FPSQ_ERR_STATE;
  }
  hipStream_t s = h->stream;
  const int64_t n = h->n, m = h->m;
  if (!h->mk_ready) {
    double** lv[] = {&h->mk_long.Y, &h->mk_long.R1, &h->mk_long.R2, &h->mk_long.W1, &h->mk_long.W2, &h->mk_long.X};
    for (auto p : lv)
      if (int rc = dalloc(h, p, 2 * (size_t)n)) return rc;
    double** sv[] = {&h->mk_short.Y, &h->mk_short.R1, &h->mk_short.R2, &h->mk_short.W1, &h->mk_short.W2, &h->mk_short.X};
    for (auto p : sv)
      if (int rc = dalloc(h, p, 2 * (size_t)m)) return rc;
    h->mk_gl = (int)((n + kMkPerBlock - 1) / kMkPerBlock);
    h->mk_gs = (int)((m + kMkPerBlock - 1) / kMkPerBlock);
    for (int l = 0; l < 2; ++l)
      if (int rc = dalloc(h, &h->mk_part[l], (size_t)(h->mk_gl + h->mk_gs))) return rc;
    if (int rc = dalloc(h, &h->mk_state, 2)) return rc;
    h->mk_ready = true;
  }
  const int gl = h->mk_gl, gt = h->mk_gl + h->mk_gs;
  const fpsq_options& o = h->opt;
  const int64_t itmax = o.ne_itmax > 0 ? o.ne_itmax : 2 * (n + m);
  MinresParams P{0.0, o.ne_atol, o.ne_rtol, o.ne_etol, o.ne_conlim, itmax, INT32_MAX};
  hipLaunchKernelGGL(k_mk_params, dim3(2), dim3(1), 0, s, h->mk_state, P, h->delta);
  hipLaunchKernelGGL(k_mk_init, dim3(gt), dim3(kBlock), 0, s, h->mk_long, bp0, bp1, n, h->mk_short, bq0, bq1, m, gl,
                     h->mk_part[0], h->mk_part[1]);
  h->launches += 2;
  MinresState* S0 = h->mk_state;
  MinresState* S1 = h->mk_state + 1;
  for (int l = 0; l < 2; ++l) {
    h->prog_host[l].iter = 0;
    h->prog_host[l].done = 0;
    h->hstats[l] = fpsq_stats{};
  }
  auto sargs = [&](int kind, int l, int it) {
    StepArgs a{};
    a.kind = kind;
    a.it = it;
    a.state = h->mk_state + l;
    a.p0 = h->mk_part[l];
    a.n0 = gt;
    a.p1 = nullptr;
    a.n1 = 0;
    a.prog = h->prog_dev + l;
    a.host_stats = h->hstats_dev + l;
    return a;
  };
  launch_step_raw(h, sargs(STEP_MINRES_BEGIN, 0, 0), sargs(STEP_MINRES_BEGIN, 1, 0));
  int64_t it = 0, chunk = 8;
  int rc = 0;
  while (true) {
    for (int64_t k = 0; k < chunk && it < itmax; ++k) {
      ++it;
      // y = K r2 / beta: long part through A', short part through A (both read the pair r2, write the pair y)
      launch_spmv<2>(h, TAG_AT, h->mk_short.R2, h->mk_long.R2, h->mk_long.Y, &S0->ctlT, &S1->ctlT, nullptr);
      launch_spmv<2>(h, TAG_A, h->mk_long.R2, h->mk_short.R2, h->mk_short.Y, &S0->ctl, &S1->ctl, nullptr);
      hipLaunchKernelGGL(k_mk_stage<1>, dim3(gt), dim3(kBlock), 0, s, &S0->ctl, &S1->ctl, (int)it, h->mk_long, n, h->mk_short,
                         m, gl, h->mk_part[0], h->mk_part[1]);
      launch_step_raw(h, sargs(STEP_MINRES_A, 0, (int)it), sargs(STEP_MINRES_A, 1, (int)it));
      hipLaunchKernelGGL(k_mk_stage<2>, dim3(gt), dim3(kBlock), 0, s, &S0->ctl, &S1->ctl, (int)it, h->mk_long, n, h->mk_short,
                         m, gl, h->mk_part[0], h->mk_part[1]);
      launch_step_raw(h, sargs(STEP_MINRES_B, 0, (int)it), sargs(STEP_MINRES_B, 1, (int)it));
      hipLaunchKernelGGL(k_mk_stage<3>, dim3(gt), dim3(kBlock), 0, s, &S0->ctl, &S1->ctl, (int)it, h->mk_long, n, h->mk_short,
                         m, gl, h->mk_part[0], h->mk_part[1]);
      launch_step_raw(h, sargs(STEP_MINRES_C, 0, (int)it), sargs(STEP_MINRES_C, 1, (int)it));
      h->launches += 3;
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      h->err = std::string("minres_k: ") + hipGetErrorString(e);
      rc = FPSQ_ERR_HIP;
      break;
    }
    if ((h->prog_host[0].done && h->prog_host[1].done) || it >= itmax) break;
    chunk = std::min<int64_t>(chunk * 2, 64);
  }
  if (rc) return rc;
  if (!(h->prog_host[0].done && h->prog_host[1].done)) {  // (the mapped words lag: read the states)
    MinresState hs[2];
    HIPCHK(h, hipMemcpy(hs, h->mk_state, sizeof hs, hipMemcpyDeviceToHost));
    for (int l = 0; l < 2; ++l) h->hstats[l] = hs[l].stats;
  }
  hipLaunchKernelGGL(k_mk_unpack, dim3(ew_grid(n)), dim3(kBlock), 0, s, h->mk_long.X, p0, p1, n);
  hipLaunchKernelGGL(k_mk_unpack, dim3(ew_grid(m)), dim3(kBlock), 0, s, h->mk_short.X, q0, q1, m);
  h->launches += 2;
  return 0;
}

// CRAIG without x in its loop (one GPU; FPSQ_CRAIG_X=1: keep the recurrence; LNLQ keeps it: its x is not A'y at the LQ point; sharded
// handles keep it): see two_mixed_device
constexpr double kMixedXSign = -1.0;  // solve_two_mixed hands out p2 = -x of the least-norm solve (src/solve_linear_system.jl:132-133)
inline bool craig_x_from_y(fpsq_handle h) {
  return h->opt.kkt_method != FPSQ_KKT_MINRES_K && h->opt.ln_method != FPSQ_LN_LNLQ && !h->comm && !h->craig_x;
}

// device-side solve_two_mixed: g (n), c (m) device pointers; results left in h->p1, h->Lx[0] (q1), h->Cx (p2), h->Cy (q2)
// defer_p1: the caller forms p1 = g - A'q1 itself (qp_objgrad pairs that product with A'c in one two-RHS launch)
// defer_p2 (only where craig_x_from_y): the caller's tail forms p2 = -A'q2 itself, in the same launch (GradEpi::y2)
// affine_shift != null (fast start): c is NOT formed yet; CRAIG's right-hand side -(A z - shift), z in the long pair's
// CRAIG lane, comes out of the LSQR start-up product and A z - shift is left in `c` (see run_krylov)
int two_mixed_device(fpsq_handle h, const double* g, double* c, bool defer_p1 = false,
                     const double* affine_shift = nullptr, const TailFn* tail = nullptr, const RunRequest& req = {},
                     bool defer_p2 = false) {
  if (h->opt.kkt_method == FPSQ_KKT_MINRES_K) {
    if (defer_p1 || affine_shift || tail) {
      h->err = "kkt_method = MINRES_K serves fpsq_solve_two_mixed / fpsq_solve_two_least_squares / fpsq_ys_gs only";
      return FPSQ_ERR_STATE;
    }
    // K [p1; q1] = [g; 0], K [p2; q2] = [0; c]
    return minres_k_device(h, g, nullptr, nullptr, c, h->p1, h->Lx[0], h->Cx, h->Cy);
  }
  Lane lanes[2];
  // (q1, stats1) = solve_least_square(qds, Aop', rhs1, sqrt(delta))      src/solve_linear_system.jl:123
  lanes[0].kind = LANE_LSQR;
  lanes[0].rhs = g;
  lanes[0].lambda = std::sqrt(h->delta);
  lanes[0].x = h->Lx[0];
  lanes[0].st = &h->hstats[0];
  // (p2, q2, stats2) = solve_least_norm(qds, Aop, -rhs2, delta); p2 = -p2 :132-133
  lanes[1].kind = h->opt.ln_method == FPSQ_LN_LNLQ ? LANE_LNLQ : LANE_CRAIG;
  lanes[1].rhs = c;
  lanes[1].rhs_scale = -1.0;
  if (affine_shift) {
    lanes[0].preloaded = true;
    lanes[1].affine_shift = affine_shift;
    lanes[1].affine_out = c;
  }
  lanes[1].delta = h->delta;
  lanes[1].xsign = kMixedXSign;
  // One GPU: CRAIG does not carry x through its loop.  Every CRAIG iterate satisfies x_k = A'y_k (first block row of
  // [-I A'; A delta I][x; y] = [0; b], with or without the regularisation), nothing in the loop reads x -- the stopping tests use
  // the scalar ||x||^2 -- and the recurrence costs 3 passes over n per iteration (5 with w2, delta != 0) that ride in the A
  // product.  p2 = xsign A'q2 is formed ONCE, behind the loop and under the tail's gates, from the final y: by the same one-lane
  // product (k_spmv<1, ..>) -- or, at the end of an evaluation, inside the launch of the tail's two-lane product A'[q1, c], whose
  // workgroups sum the rows of A'q2 the way that kernel does (GradEpi::y2, defer_p2) -- so that p2 / v is bitwise the same
  // whichever entry point or tail variant asks for it.
  const bool x_from_y = craig_x_from_y(h);
  lanes[1].x = x_from_y ? nullptr : h->Cx;
  lanes[1].y = h->Cy;
  lanes[1].st = &h->hstats[1];
  // p1 = rhs1 - Aop' q1                                                   :126-127
  // (neither deferred -- fpsq_solve_two_mixed, fpsq_ys_gs, an evaluation with rho = 0 -- and column-sorted padded A' blocks: the two share ONE stream of the matrix)
  const bool seam = x_from_y && !defer_p2 && !defer_p1 && h->tail_lanes == 3 && !h->craig_v_alone && h->AT.sorted && h->AT.padded;
  TailFn full = [&](const TailCtx& t) -> int {
    if (seam) {
      launch_at_seam(h, h->Lx[0], g, h->p1, h->Cy, lanes[1].xsign, h->Cx, t.gates);
      return tail ? (*tail)(t) : 0;
    }
    if (x_from_y && !defer_p2)
      if (int rc = at_product_const(h, lanes[1].xsign, h->Cy, 0.0, nullptr, h->Cx, t.gates)) return rc;
    if (!defer_p1)
      if (int rc = at_product_const(h, -1.0, h->Lx[0], 1.0, g, h->p1, t.gates)) return rc;
    return tail ? (*tail)(t) : 0;
  };
  RunResult r;
  if (int rc = run_lanes(h, lanes, 2, tail ? &full : nullptr, req, &r)) return rc;
  if (!r.tail_was_run)
    if (int rc = full(TailCtx{Gates{}, r.flush})) return rc;
  return 0;
}

// device-side solve_two_least_squares: results in h->p1, h->Lx[0], h->p2b, h->Lx[1]
int two_least_squares_device(fpsq_handle h, const double* r1, const double* r2, const TailFn* tail = nullptr) {
  if (h->opt.kkt_method == FPSQ_KKT_MINRES_K) {
    if (tail) {
      h->err = "kkt_method = MINRES_K serves fpsq_solve_two_mixed / fpsq_solve_two_least_squares / fpsq_ys_gs only";
      return FPSQ_ERR_STATE;
    }
    return minres_k_device(h, r1, nullptr, r2, nullptr, h->p1, h->Lx[0], h->p2b, h->Lx[1]);
  }
  Lane lanes[2];
  const double* rhs[2] = {r1, r2};
  for (int l = 0; l < 2; ++l) {
    lanes[l].kind = LANE_LSQR;
    lanes[l].rhs = rhs[l];
    lanes[l].lambda = std::sqrt(h->delta);
    lanes[l].x = h->Lx[l];
    lanes[l].st = &h->hstats[l];
  }
  // src/solve_linear_system.jl:90-91 and :99-100
  TailFn full = [&](const TailCtx& t) -> int {
    if (int rc = at_product_const(h, -1.0, h->Lx[0], 1.0, r1, h->p1, t.gates)) return rc;
    if (int rc = at_product_const(h, -1.0, h->Lx[1], 1.0, r2, h->p2b, t.gates)) return rc;
    return tail ? (*tail)(t) : 0;
  };
  RunResult r;
  if (int rc = run_lanes(h, lanes, 2, tail ? &full : nullptr, {}, &r)) return rc;
  if (!r.tail_was_run)
    if (int rc = full(TailCtx{Gates{}, r.flush})) return rc;
  return 0;
}

}  // namespace

// ===================================================================================== C ABI

// One-launch iterations and workgroup slots.  The waiting workgroups of a fused launch hold slots that the workgroups they wait for
// may still need.  WITHIN ONE LAUNCH that cannot deadlock: every dependence points to a workgroup earlier in the grid, a queue
// dispatches its grid in order (workgroup i through XCD i mod 8, in order within the XCD), and the leaders are one per lane on
// EVERY XCD -- so whatever a running workgroup waits for has been dispatched ahead of it on the XCD that dispatches it, and
// the earliest unfinished workgroup of the grid waits for nothing.  ACROSS LAUNCHES that argument does not hold -- two handles
// of this process iterating from two host threads are two queues, exactly like two processes: each queue's waiting workgroups
// can fill slots the OTHER queue's not-yet-dispatched workgroups need.  No circular wait was ever observed inside one process
// (tools/fuse_soak_two.py: 2.4 M fused launches of two handles sharing the device), three ranks rehearsed on ONE GPU did run into
// it; the answer is the same for both: every wait is bounded, the call ends in FPSQ_ERR_TIMEOUT with every kernel gone, the
// handle keeps two launches per iteration from then on (ride_failed -- their waits involve the leaders only) and the call is
// REPEATED once -- its inputs are untouched -- so the caller sees a delay and fpsq_info.fuse_fallbacks, not an error.
template <class F>
int with_fuse_fallback(fpsq_handle h, F&& call) {
  int rc = call();
  // (a rank of several cannot repeat a call on its own -- its peers are not repeating theirs: there the expired wait is the call's
  // result, FPSQ_ERR_TIMEOUT on this rank and, through the peers' own bounded waits, on the others; the job decides what next --
  // bench.py starts over on the collectives.  Their waits are long for that reason: RideArgs::more.)
  if (rc == FPSQ_ERR_TIMEOUT && h && h->fuse_fell_back && !(h->comm && h->comm->nranks > 1)) {
    h->fuse_fell_back = false;
    h->info.fuse_fallbacks++;  // (fpsq_info: a benchmark or a test sees that it happened)
    if (h->verbose)
      std::fprintf(stderr, "fpsq: a bounded wait of a one-launch iteration expired (is the GPU shared with other processes?); this handle "
                           "continues with two launches per iteration, the call is repeated\n");
    rc = call();
  }
  if (h) h->fuse_fell_back = false;
  return rc;
}

extern "C" {

const char* fpsq_version(void) { return "fpsq 0.1.0 (gfx950)"; }

void fpsq_default_options(int64_t n, int64_t m, fpsq_options* o) {
  const double se = std::sqrt(2.220446049250313e-16);
  std::memset(o, 0, sizeof *o);
  o->ls_atol = se;
  o->ls_rtol = se;
  o->ls_itmax = 5 * (m + n);
  o->ln_atol = se;
  o->ln_rtol = se;
  o->ln_btol = se;
  o->ln_conlim = 1.0 / se;
  o->ln_itmax = 5 * (m + n);
  o->ne_atol = se;
  o->ne_rtol = se;
  o->ne_etol = se;
  o->ne_itmax = 0;
  o->ne_conlim = 1.0 / se;
  o->ls_axtol = se;
  o->ls_btol = se;
  o->ls_etol = se;
  o->ls_conlim = 1.0 / se;
  o->fuse_two_rhs = 1;
  o->lookahead = 4;
  o->device = 0;
}

const char* fpsq_last_error(fpsq_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int fpsq_create(fpsq_handle* out, int64_t n, int64_t m, const fpsq_options* opts) {
  if (!out || n <= 0 || m <= 0 || n >= INT32_MAX || m >= INT32_MAX) {
    g_create_error = "fpsq_create: bad arguments";
    return FPSQ_ERR_ARG;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    g_create_error = std::string("fpsq_create: no HIP device (") + hipGetErrorString(e) +
                     "); libfpsq has no CPU fallback";
    return FPSQ_ERR_HIP;
  }
  fpsq_handle h = new fpsq_solver_s();
  h->n = n;
  h->m = m;
  if (opts) h->opt = *opts; else fpsq_default_options(n, m, &h->opt);
  auto fail = [&](const char* what, hipError_t err) {
    g_create_error = std::string("fpsq_create: ") + what + ": " + hipGetErrorString(err);
    delete h;
    return FPSQ_ERR_HIP;
  };
  if ((e = hipSetDevice(h->opt.device)) != hipSuccess) return fail("hipSetDevice", e);
  if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
  if ((e = hipHostMalloc((void**)&h->prog_host, 4 * sizeof(Progress), hipHostMallocMapped | hipHostMallocCoherent)) !=
      hipSuccess)
    return fail("hipHostMalloc", e);
  std::memset(h->prog_host, 0, 4 * sizeof(Progress));
  if ((e = hipHostGetDevicePointer((void**)&h->prog_dev, h->prog_host, 0)) != hipSuccess)
    return fail("hipHostGetDevicePointer", e);
  if ((e = hipHostMalloc((void**)&h->hstats, 4 * sizeof(fpsq_stats), hipHostMallocMapped | hipHostMallocCoherent)) !=
      hipSuccess)
    return fail("hipHostMalloc", e);
  if ((e = hipHostMalloc((void**)&h->hscal, 16 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent)) !=
      hipSuccess)
    return fail("hipHostMalloc", e);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->opt.device) == hipSuccess && prop.multiProcessorCount > 0) {
      h->resident_wgs = 4 * prop.multiProcessorCount;
      int xccs = 0;
      if (hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, h->opt.device) != hipSuccess) {
        (void)hipGetLastError();
        xccs = 0;
      }
      int per_cu = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_minres_mid, kBlock, 0) == hipSuccess && per_cu > 0)
        h->mmid_cap = per_cu * prop.multiProcessorCount;
      else
        (void)hipGetLastError();
      const std::string arch = prop.gcnArchName;
      h->fuse_hw_ok = xccs == 8 && (arch.rfind("gfx950", 0) == 0 || arch.rfind("gfx942", 0) == 0);
    }
  }
  read_switches(h);
  std::memset(h->hstats, 0, 4 * sizeof(fpsq_stats));
  std::memset(h->hscal, 0, 16 * sizeof(double));
  if ((e = hipHostGetDevicePointer((void**)&h->hstats_dev, h->hstats, 0)) != hipSuccess)
    return fail("hipHostGetDevicePointer", e);
  if ((e = hipHostGetDevicePointer((void**)&h->hscal_dev, h->hscal, 0)) != hipSuccess)
    return fail("hipHostGetDevicePointer", e);
  hipEventCreate(&h->ev0);
  hipEventCreate(&h->ev1);
  void* p = nullptr;
  const size_t state_bytes = sizeof(LsqrState) * 6 + sizeof(CraigState) * 3 + sizeof(MinresState) * 2 + sizeof(LnlqState) * 3 +
                             5 * sizeof(LaneCtl) + 64 * sizeof(double);
  if ((e = hipMalloc(&p, state_bytes)) != hipSuccess) return fail("hipMalloc", e);
  h->allocs.push_back(p);
  hipMemset(p, 0, state_bytes);
  {
    void* q = nullptr;
    // (a record copy of 64 words per XCC; a second record for the mid leaders of fused iterations)
    if ((e = hipMalloc(&q, 2 * 8 * 512 + 64)) != hipSuccess) return fail("hipMalloc", e);
    h->allocs.push_back(q);
    hipMemset(q, 0, 2 * 8 * 512 + 64);
    h->ride_rec = (unsigned long long*)q;
    h->ride_rec2 = h->ride_rec + 512;
  }
  char* cp = (char*)p;
  h->lsqr[0] = (LsqrState*)cp;
  h->lsqr[1] = h->lsqr[0] + 1;
  cp += sizeof(LsqrState) * 2;
  h->craig = (CraigState*)cp;
  cp += sizeof(CraigState);
  h->lsqr_alt[0] = (LsqrState*)cp;
  h->lsqr_alt[1] = h->lsqr_alt[0] + 1;
  cp += sizeof(LsqrState) * 2;
  h->craig_alt = (CraigState*)cp;
  cp += sizeof(CraigState);
  h->minres = (MinresState*)cp;
  cp += sizeof(MinresState);
  h->lnlq = (LnlqState*)cp;
  cp += sizeof(LnlqState);
  h->lnlq_alt = (LnlqState*)cp;
  cp += sizeof(LnlqState);
  h->minres_alt = (MinresState*)cp;
  cp += sizeof(MinresState);
  h->state3[0] = cp;  // (two LSQR states)
  cp += sizeof(LsqrState) * 2;
  h->state3[1] = cp;
  cp += sizeof(CraigState);
  h->state3[2] = cp;
  cp += sizeof(LnlqState);
  h->ctl_tmp = (LaneCtl*)cp;
  cp += sizeof(LaneCtl);
  h->ctl_raw = (LaneCtl*)cp;
  cp += sizeof(LaneCtl);
  h->ctl_pm = (LaneCtl*)cp;
  cp += sizeof(LaneCtl);
  h->ctl_mp = (LaneCtl*)cp;
  cp += sizeof(LaneCtl);
  h->ctl_m0 = (LaneCtl*)cp;
  cp += sizeof(LaneCtl);
  h->dscal = (double*)cp;
  h->comm_scal = h->dscal + 32;
  {
    LaneCtl raw{};
    raw.ca = 1.0;
    raw.cb = 0.0;
    raw.upd_iter = -1;
    hipMemcpy(h->ctl_raw, &raw, sizeof raw, hipMemcpyHostToDevice);
    raw.ca = 1.0;
    raw.cb = -1.0;
    hipMemcpy(h->ctl_pm, &raw, sizeof raw, hipMemcpyHostToDevice);
    raw.ca = -1.0;
    raw.cb = 1.0;
    hipMemcpy(h->ctl_mp, &raw, sizeof raw, hipMemcpyHostToDevice);
    raw.ca = -1.0;
    raw.cb = 0.0;
    hipMemcpy(h->ctl_m0, &raw, sizeof raw, hipMemcpyHostToDevice);
  }
  hipDeviceSynchronize();
  *out = h;
  return FPSQ_OK;
}

int fpsq_destroy(fpsq_handle h) {
  if (!h) return FPSQ_ERR_ARG;
  if (h->host_trace && h->ht_calls > 0) {
    static const char* nm[12] = {"between calls", "entry->inputs ordered", "->first launch", "->krylov start", "->krylov end",
                                 "->epilogue enqueued", "->synchronised", "->exit", "", "", "", ""};
    std::fprintf(stderr, "fpsq host trace (%lld qp_objgrad calls), us per call:", (long long)h->ht_calls);
    for (int k = 0; k < 8; ++k) std::fprintf(stderr, "  %s %.1f", nm[k], 1e6 * h->ht_sum[k] / (double)h->ht_calls);
    std::fprintf(stderr, "\n");
  }
  hipSetDevice(h->opt.device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->fuse_probe_buf && !h->fuse_probe_path.empty()) {  // developer probe: "grid n0 n1 .. n5" then one line of four stamps per workgroup
    std::vector<unsigned long long> st((size_t)h->fuse_probe_grid * 4);
    hipMemcpy(st.data(), h->fuse_probe_buf, st.size() * 8, hipMemcpyDeviceToHost);
    if (FILE* f = std::fopen(h->fuse_probe_path.c_str(), "w")) {
      std::fprintf(f, "%d", h->fuse_probe_grid);
      for (int v : h->fuse_probe_layout) std::fprintf(f, " %d", v);
      std::fprintf(f, "\n");
      for (int i = 0; i < h->fuse_probe_grid; ++i)
        std::fprintf(f, "%llu %llu %llu %llu\n", st[4 * (size_t)i], st[4 * (size_t)i + 1], st[4 * (size_t)i + 2], st[4 * (size_t)i + 3]);
      std::fclose(f);
    }
  }
  delete h->comm;
  for (void* p : h->allocs) hipFree(p);
  for (auto& e : h->ev_pool) {
    hipEventDestroy(e.a);
    hipEventDestroy(e.b);
  }
  if (h->ev0) hipEventDestroy(h->ev0);
  if (h->ev1) hipEventDestroy(h->ev1);
  if (h->ev_in) hipEventDestroy(h->ev_in);
  if (h->ev_out) hipEventDestroy(h->ev_out);
  if (h->prog_host) hipHostFree(h->prog_host);
  if (h->hstats) hipHostFree(h->hstats);
  if (h->hscal) hipHostFree(h->hscal);
  if (h->own_stream && h->own_stream != h->stream) {  // (an adopted stream is the caller's)
    hipStreamDestroy(h->own_stream);
  } else if (h->stream && !h->adopted) {
    hipStreamDestroy(h->stream);
  }
  delete h;
  return FPSQ_OK;
}

int fpsq_set_jacobian_structure_csr(fpsq_handle h, const int32_t* rowptr, const int32_t* colind) {
  if (!h || !rowptr || h->have_structure) {
    if (h) h->err = "set_jacobian_structure: bad arguments or structure already set";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(h->opt.device);
  HostCsr HA;
  HA.nrows = h->m;
  HA.ncols = h->n;
  HA.rowptr.resize(h->m + 1);
  HIPCHK(h, hipMemcpy(HA.rowptr.data(), rowptr, (size_t)(h->m + 1) * 4, hipMemcpyDefault));
  const int64_t nnz = HA.rowptr[h->m];
  if (HA.rowptr[0] != 0 || nnz < 0) {
    h->err = "set_jacobian_structure_csr: rowptr must be 0-based";
    return FPSQ_ERR_ARG;
  }
  HA.colind.resize(nnz);
  if (nnz) HIPCHK(h, hipMemcpy(HA.colind.data(), colind, (size_t)nnz * 4, hipMemcpyDefault));
  for (int64_t i = 0; i < h->m; ++i)
    if (HA.rowptr[i + 1] < HA.rowptr[i]) {
      h->err = "set_jacobian_structure_csr: rowptr not monotone";
      return FPSQ_ERR_ARG;
    }
  for (int64_t k = 0; k < nnz; ++k)
    if (HA.colind[k] < 0 || HA.colind[k] >= h->n) {
      h->err = "set_jacobian_structure_csr: column index out of range";
      return FPSQ_ERR_ARG;
    }
  h->nnz_in = nnz;
  return finish_structure(h, HA);
}

int fpsq_set_jacobian_structure_coo(fpsq_handle h, int64_t nnz, const int64_t* rows, const int64_t* cols,
                                    int32_t index_base) {
  if (!h || nnz < 0 || nnz >= INT32_MAX || (nnz > 0 && (!rows || !cols)) || h->have_structure) {
    if (h) h->err = "set_jacobian_structure_coo: bad arguments or structure already set";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(h->opt.device);
  std::vector<int64_t> r(nnz), c(nnz);
  if (nnz) {
    HIPCHK(h, hipMemcpy(r.data(), rows, (size_t)nnz * 8, hipMemcpyDefault));
    HIPCHK(h, hipMemcpy(c.data(), cols, (size_t)nnz * 8, hipMemcpyDefault));
  }
  const int64_t m = h->m, n = h->n;
  std::vector<int32_t> cnt(m + 1, 0);
  for (int64_t k = 0; k < nnz; ++k) {
    r[k] -= index_base;
    c[k] -= index_base;
    if (r[k] < 0 || r[k] >= m || c[k] < 0 || c[k] >= n) {
      h->err = "set_jacobian_structure_coo: index out of range";
      return FPSQ_ERR_ARG;
    }
    cnt[r[k] + 1]++;
  }
  for (int64_t i = 0; i < m; ++i) cnt[i + 1] += cnt[i];
  // bucket by row (stable), then sort each row by column (stable: duplicates keep the caller's order)
  std::vector<int32_t> order(nnz);
  {
    std::vector<int32_t> next(cnt.begin(), cnt.end() - 1);
    for (int64_t k = 0; k < nnz; ++k) order[next[r[k]]++] = (int32_t)k;
  }
  for (int64_t i = 0; i < m; ++i)
    std::stable_sort(order.begin() + cnt[i], order.begin() + cnt[i + 1],
                     [&](int32_t a, int32_t b) { return c[a] < c[b]; });
  HostCsr HA;
  HA.nrows = m;
  HA.ncols = n;
  HA.rowptr.assign(m + 1, 0);
  std::vector<int32_t> slotptr;
  slotptr.push_back(0);
  for (int64_t i = 0; i < m; ++i) {
    for (int32_t k = cnt[i]; k < cnt[i + 1]; ++k) {
      const int64_t col = c[order[k]];
      if (k > cnt[i] && col == c[order[k - 1]]) {
        slotptr.back() = k + 1;  // duplicate: extend the current slot
      } else {
        HA.colind.push_back((int32_t)col);
        slotptr.push_back(k + 1);
      }
    }
    HA.rowptr[i + 1] = (int32_t)HA.colind.size();
  }
  const bool dup = (int64_t)HA.colind.size() != nnz;
  h->nnz_in = nnz;
  if (int rc = dalloc(h, &h->in_perm, (size_t)nnz)) return rc;
  if (int rc = dalloc(h, &h->in_vals, (size_t)nnz)) return rc;
  if (nnz) HIPCHK(h, hipMemcpy(h->in_perm, order.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
  if (dup) {
    if (int rc = dalloc(h, &h->in_slotptr, slotptr.size())) return rc;
    HIPCHK(h, hipMemcpy(h->in_slotptr, slotptr.data(), slotptr.size() * 4, hipMemcpyHostToDevice));
  }
  return finish_structure(h, HA);
}

int fpsq_set_jacobian_values(fpsq_handle h, const double* vals) {
  if (!h || !h->have_structure || (!vals && h->nnz_in > 0)) {
    if (h) h->err = "set_jacobian_values: structure not set or null values";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(h->opt.device);
  hipStream_t s = h->stream;
  order_inputs(h);
  const bool on_dev = h->nnz_in > 0 && on_this_device(h, vals);
  if (h->nnz_in > 0 && h->refresh_3pass) {
    // rounds 1-3: a copy into the staging array, then one grid-stride gather per stored copy
    if (h->in_perm) {
      HIPCHK(h, hipMemcpyAsync(h->in_vals, vals, (size_t)h->nnz_in * 8, hipMemcpyDefault, s));
      if (h->in_slotptr)
        hipLaunchKernelGGL(k_gather_sum, dim3(ew_grid(h->nnz)), dim3(kBlock), 0, s, h->in_vals, h->in_perm,
                           h->in_slotptr, h->A.vals, h->nnz);
      else
        hipLaunchKernelGGL(k_gather, dim3(ew_grid(h->nnz)), dim3(kBlock), 0, s, h->in_vals, h->in_perm, h->A.vals,
                           h->nnz);
    } else {
      HIPCHK(h, hipMemcpyAsync(h->A.vals, vals, (size_t)h->nnz * 8, hipMemcpyDefault, s));
    }
    if (h->AT.nstore > 0)
      hipLaunchKernelGGL(k_gather, dim3(ew_grid(h->AT.nstore)), dim3(kBlock), 0, s, h->A.vals, h->permT, h->AT.vals,
                         h->AT.nstore);
    if (h->RA.ok)
      hipLaunchKernelGGL(k_gather, dim3(ew_grid(h->RA.nstore)), dim3(kBlock), 0, s, h->A.vals, h->RA.vperm, h->RA.vals,
                         h->RA.nstore);
  } else if (h->nnz_in > 0) {
    // ONE launch writes every stored copy (k_refresh).  Where the gathers read from:
    //   CSR input              the caller's array in place when it lives on this GPU, else its copy in the CSR array
    //   COO, no duplicates     the caller's array in place / its staged copy, through permutations composed at set-up
    //   COO with duplicates    the CSR array, after the slots were summed into it (one more pass; fixed order)
    const double* src = vals;
    bool csr_is_src = false;  // (the CSR array already holds the values the gathers read)
    if (h->in_perm && h->in_slotptr) {
      const double* coo = vals;
      if (!on_dev) {
        HIPCHK(h, hipMemcpyAsync(h->in_vals, vals, (size_t)h->nnz_in * 8, hipMemcpyDefault, s));
        coo = h->in_vals;
      }
      hipLaunchKernelGGL(k_gather_sum, dim3(ew_grid(h->nnz)), dim3(kBlock), 0, s, coo, h->in_perm, h->in_slotptr, h->A.vals,
                         h->nnz);
      src = h->A.vals;
      csr_is_src = true;
    } else if (!on_dev) {
      double* stage = h->in_perm ? h->in_vals : h->A.vals;
      HIPCHK(h, hipMemcpyAsync(stage, vals, (size_t)h->nnz_in * 8, hipMemcpyDefault, s));
      src = stage;
      csr_is_src = !h->in_perm;
    }
    const RefreshSeg none{nullptr, nullptr, 0, 0, 0};
    auto seg = [](double* out, const int32_t* perm, int64_t n) {
      return RefreshSeg{out, perm, n, (int32_t)((n + kRefreshChunk - 1) / kRefreshChunk), 0};
    };
    const RefreshSeg sT = h->AT.nstore > 0 ? seg(h->AT.vals, h->permT, h->AT.nstore) : none;
    const RefreshSeg sR = h->RA.ok ? seg(h->RA.vals, h->RA.vperm, h->RA.nstore) : none;
    // the CSR array itself: only when a product reads it (no row-group copy of A) and it is not the source already
    const RefreshSeg sC = (!h->RA.ok && !csr_is_src) ? seg(h->A.vals, h->perms_to_input ? h->in_perm : nullptr, h->nnz) : none;
    if (std::getenv("FPSQ_REFRESH_SPLIT")) {  // (developer: one launch per segment, to time them apart)
      for (const RefreshSeg* q : {&sT, &sR, &sC})
        if (q->nchunk) hipLaunchKernelGGL(k_refresh, dim3((q->nchunk + 7) / 8 * 8), dim3(kBlock), 0, s, src, *q, none, none, (q->nchunk + 7) / 8);
    } else {
      const int per_xcd = (sT.nchunk + sR.nchunk + sC.nchunk + 7) / 8;
      hipLaunchKernelGGL(k_refresh, dim3(per_xcd * 8), dim3(kBlock), 0, s, src, sT, sR, sC, per_xcd);
    }
  }
  if (on_dev && h->adopted) {
    // (the gathers were enqueued on the caller's own stream)
  } else if (on_dev && h->in_stream_on) {
    // device-resident values on a registered stream: no host synchronisation -- the caller's stream is made to wait for
    // the gathers that read its array (it may overwrite the array with the next Jacobian), the solves that follow run on
    // the library's stream behind them
    if (!h->ev_out) HIPCHK(h, hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(h->ev_out, s));
    HIPCHK(h, hipStreamWaitEvent(h->in_stream, h->ev_out, 0));
  } else {
    HIPCHK(h, hipStreamSynchronize(s));
  }
  h->have_values = true;
  return FPSQ_OK;
}

int fpsq_set_input_stream(fpsq_handle h, int32_t enabled, void* hip_stream) {
  if (!h) return FPSQ_ERR_ARG;
  hipSetDevice(h->opt.device);
  if (enabled && !h->ev_in) HIPCHK(h, hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
  if (h->adopt_streams && (!h->comm || h->comm->nranks == 1)) {  // (a communicator of one rank has no peers)
    if (enabled && h->adopted && h->stream == (hipStream_t)hip_stream) return FPSQ_OK;  // (registered again: nothing to do)
    // everything enqueued so far is on the stream in use: finish it, then move
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!h->own_stream) h->own_stream = h->stream;
    h->adopted = enabled != 0;
    h->stream = h->adopted ? (hipStream_t)hip_stream : h->own_stream;
  }
  h->in_stream_on = enabled != 0;
  h->in_stream = (hipStream_t)hip_stream;
  return FPSQ_OK;
}

int fpsq_set_output_ordering(fpsq_handle h, int32_t stream_ordered) {
  if (!h) return FPSQ_ERR_ARG;
  hipSetDevice(h->opt.device);
  if (stream_ordered && !h->ev_out) HIPCHK(h, hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
  h->out_ordered = stream_ordered != 0;
  return FPSQ_OK;
}

int fpsq_set_delta(fpsq_handle h, double delta) {
  if (!h || !(delta >= 0.0)) {
    if (h) h->err = "set_delta: delta must be >= 0";
    return FPSQ_ERR_ARG;
  }
  h->delta = delta;
  return FPSQ_OK;
}

static int impl_solve_two_mixed(fpsq_handle h, const double* rhs1, const double* rhs2, double* p1, double* q1, double* p2,
                         double* q2, fpsq_stats st[2]) {
  if (int rc = check_ready(h)) return rc;
  if (!rhs1 || !rhs2 || !p1 || !q1 || !p2 || !q2 || !st) {
    h->err = "solve_two_mixed: null argument";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(h->opt.device);
  hipStream_t s = h->stream;
  order_inputs(h);
  const size_t nb = (size_t)h->n * 8, mb = (size_t)h->m * 8;
  HIPCHK(h, hipMemcpyAsync(h->in_n1, rhs1, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(h->in_m, rhs2, mb, hipMemcpyDefault, s));
  call_begin(h);
  if (int rc = two_mixed_device(h, h->in_n1, h->in_m)) return rc;
  HIPCHK(h, hipMemcpyAsync(p1, h->p1, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(q1, h->Lx[0], mb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(p2, h->Cx, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(q2, h->Cy, mb, hipMemcpyDefault, s));
  if (int rc = call_end(h)) return rc;
  st[0] = h->hstats[0];
  st[1] = h->hstats[1];
  return soft_rc(st);
}

static int impl_solve_two_least_squares(fpsq_handle h, const double* rhs1, const double* rhs2, double* p1, double* q1,
                                 double* p2, double* q2, fpsq_stats st[2]) {
  if (int rc = check_ready(h)) return rc;
  if (!rhs1 || !rhs2 || !p1 || !q1 || !p2 || !q2 || !st) {
    h->err = "solve_two_least_squares: null argument";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(h->opt.device);
  hipStream_t s = h->stream;
  order_inputs(h);
  const size_t nb = (size_t)h->n * 8, mb = (size_t)h->m * 8;
  HIPCHK(h, hipMemcpyAsync(h->in_n1, rhs1, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(h->in_n2, rhs2, nb, hipMemcpyDefault, s));
  call_begin(h);
  if (int rc = two_least_squares_device(h, h->in_n1, h->in_n2)) return rc;
  HIPCHK(h, hipMemcpyAsync(p1, h->p1, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(q1, h->Lx[0], mb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(p2, h->p2b, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(q2, h->Lx[1], mb, hipMemcpyDefault, s));
  if (int rc = call_end(h)) return rc;
  st[0] = h->hstats[0];
  st[1] = h->hstats[1];
  return soft_rc(st);
}

static int impl_solve_two_extras(fpsq_handle h, const double* rhs1, const double* rhs2, double* out1, double* out2,
                          fpsq_stats st[2]) {
  if (int rc = check_ready(h)) return rc;
  if (!rhs1 || !rhs2 || !out1 || !out2 || !st) {
    h->err = "solve_two_extras: null argument";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(h->opt.device);
  hipStream_t s = h->stream;
  order_inputs(h);
  const size_t nb = (size_t)h->n * 8, mb = (size_t)h->m * 8;
  HIPCHK(h, hipMemcpyAsync(h->in_n1, rhs1, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(h->in_m, rhs2, mb, hipMemcpyDefault, s));
  call_begin(h);
  const double tau = std::max(h->delta, 1e-14);  // src/solve_linear_system.jl:51
  // (invJtJJv, stats) = solve_least_square(qds, Aop', rhs1, sqrt(tau))          :53
  Lane lanes[2];
  lanes[0].kind = LANE_LSQR;
  lanes[0].rhs = h->in_n1;
  lanes[0].lambda = std::sqrt(tau);
  lanes[0].x = h->Lx[0];
  lanes[0].st = &h->hstats[0];
  // minres(JtJ, rhs2, lambda = tau)                                              :58-72
  // (fused: the MINRES recurrence shares the two products of every LSQR iteration, see run_krylov)
  lanes[1].kind = LANE_MINRES;
  lanes[1].rhs = h->in_m;
  lanes[1].lambda = tau;
  lanes[1].x = h->Mx;
  lanes[1].st = &h->hstats[1];
  if (int rc = run_lanes(h, lanes, 2)) return rc;
  HIPCHK(h, hipMemcpyAsync(out1, h->Lx[0], mb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(out2, h->Mx, mb, hipMemcpyDefault, s));
  if (int rc = call_end(h)) return rc;
  st[0] = h->hstats[0];
  st[1] = h->hstats[1];
  return soft_rc(st);
}

int fpsq_ys_gs(fpsq_handle h, const double* g, const double* c, double sigma, double* gs, double* ys, double* v,
               double* w, fpsq_stats st[2]) {
  if (int rc = check_ready(h)) return rc;
  if (!g || !c || !gs || !ys || !v || !w || !st) {
    h->err = "ys_gs: null argument";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(h->opt.device);
  hipStream_t s = h->stream;
  order_inputs(h);
  const size_t nb = (size_t)h->n * 8, mb = (size_t)h->m * 8;
  HIPCHK(h, hipMemcpyAsync(h->in_n1, g, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(h->in_m, c, mb, hipMemcpyDefault, s));
  call_begin(h);
  if (int rc = two_mixed_device(h, h->in_n1, h->in_m)) return rc;
  // src/model-Fletcherpenaltynlp.jl:244-248
  hipLaunchKernelGGL(k_gs, dim3(ew_grid(h->n)), dim3(kBlock), 0, s, h->p1, h->Cx, sigma, h->gs, h->n);
  hipLaunchKernelGGL(k_ys, dim3(ew_grid(h->m)), dim3(kBlock), 0, s, h->Lx[0], h->Cy, (const double*)nullptr, sigma, h->ys,
                     h->m, (double*)nullptr, (double*)nullptr, (double*)nullptr, (const LaneCtl*)nullptr,
                     (const LaneCtl*)nullptr, seg_none());
  h->launches += 2;
  HIPCHK(h, hipMemcpyAsync(gs, h->gs, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(ys, h->ys, mb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(v, h->Cx, nb, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(w, h->Cy, mb, hipMemcpyDefault, s));
  if (int rc = call_end(h)) return rc;
  st[0] = h->hstats[0];
  st[1] = h->hstats[1];
  return soft_rc(st);
}

int fpsq_jac_mul(fpsq_handle h, int32_t trans, double alpha, const double* x, double beta, double* y) {
  if (int rc = check_ready(h)) return rc;
  if (!x || !y) {
    h->err = "jac_mul: null argument";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(h->opt.device);
  hipStream_t s = h->stream;
  order_inputs(h);
  const size_t xb = (size_t)(trans ? h->m : h->n) * 8, yb = (size_t)(trans ? h->n : h->m) * 8;
  double* dx = trans ? h->in_m : h->in_n1;
  double* dy = trans ? h->in_n2 : h->c;
  HIPCHK(h, hipMemcpyAsync(dx, x, xb, hipMemcpyDefault, s));
  if (beta != 0.0) HIPCHK(h, hipMemcpyAsync(dy, y, yb, hipMemcpyDefault, s));
  call_begin(h);
  if (trans) {
    if (int rc = at_product_const(h, alpha, dx, beta, dy, dy)) return rc;
  } else {
    spmv_const(h, TAG_A, alpha, dx, beta, dy, dy);
  }
  HIPCHK(h, hipMemcpyAsync(y, dy, yb, hipMemcpyDefault, s));
  return call_end(h);
}

// ---------------------------------------------------------------- device-resident equality-QP model

int fpsq_qp_create(fpsq_handle h, const double* qdiag, const double* d, const double* b, fpsq_qp* out) {
  if (!h || !qdiag || !d || !b || !out) return FPSQ_ERR_ARG;
  hipSetDevice(h->opt.device);
  fpsq_qp qp = new fpsq_qp_s();
  qp->h = h;
  if (dalloc(h, &qp->q, (size_t)h->n) || dalloc(h, &qp->d, (size_t)h->n) || dalloc(h, &qp->b, (size_t)h->m)) {
    delete qp;
    return FPSQ_ERR_HIP;
  }
  HIPCHK(h, hipMemcpy(qp->q, qdiag, (size_t)h->n * 8, hipMemcpyDefault));
  HIPCHK(h, hipMemcpy(qp->d, d, (size_t)h->n * 8, hipMemcpyDefault));
  HIPCHK(h, hipMemcpy(qp->b, b, (size_t)h->m * 8, hipMemcpyDefault));
  *out = qp;
  return FPSQ_OK;
}

int fpsq_qp_destroy(fpsq_qp qp) {
  if (!qp) return FPSQ_ERR_ARG;
  delete qp;  // device arrays are owned by the solver handle's arena
  return FPSQ_OK;
}

// the single-GPU LSQR + CRAIG handle is the scope of a model with a sparse objective Hessian: in halo mode the n-vectors are
// column windows and R would need an exchange of its own; MINRES on K keeps its vectors interleaved
static int sparse_q_scope(fpsq_handle h, const char* who) {
  if (!h->comm && h->opt.kkt_method == FPSQ_KKT_LSQR_CRAIG) return FPSQ_OK;
  h->err = std::string(who) + ": a sparse objective Hessian needs a single-GPU handle with kkt_method = FPSQ_KKT_LSQR_CRAIG (this one " +
           (h->comm ? "has a communicator)" : "runs MINRES on K)");
  return FPSQ_ERR_STATE;
}

int fpsq_qp_create_csr(fpsq_handle h, const int32_t* q_rowptr, const int32_t* q_colind, const double* q_vals, const double* d,
                       const double* b, fpsq_qp* out) {
  if (!h || !q_rowptr || !d || !b || !out) return FPSQ_ERR_ARG;
  if (int rc = sparse_q_scope(h, "qp_create_csr")) return rc;
  hipSetDevice(h->opt.device);
  const int64_t n = h->n;
  auto bad = [&](const std::string& what) {
    h->err = "qp_create_csr: " + what;
    return FPSQ_ERR_ARG;
  };
  if (n >= INT32_MAX) return bad("n does not fit the 32-bit row indices of Q");
  // Q on the host, once: the checks and the split Q = diag(q) + R  (fpsq_qcsr.h)
  std::vector<int32_t> rp((size_t)n + 1);
  HIPCHK(h, hipMemcpy(rp.data(), q_rowptr, ((size_t)n + 1) * 4, hipMemcpyDefault));
  if (const std::string what = qcsr_check_rowptr(n, rp.data()); !what.empty()) return bad(what);
  const size_t nnz = (size_t)rp[n];  // (32-bit offsets: nnz(R) <= nnz(Q) < 2^31)
  if (nnz && (!q_colind || !q_vals)) return FPSQ_ERR_ARG;
  std::vector<int32_t> ci(nnz);
  std::vector<double> va(nnz);
  if (nnz) {
    HIPCHK(h, hipMemcpy(ci.data(), q_colind, nnz * 4, hipMemcpyDefault));
    HIPCHK(h, hipMemcpy(va.data(), q_vals, nnz * 8, hipMemcpyDefault));
  }
  QcsrSplit sp;
  if (const std::string what = qcsr_check_split(n, rp.data(), ci.data(), va.data(), sp); !what.empty()) return bad(what);
  fpsq_qp qp = nullptr;
  if (int rc = fpsq_qp_create(h, sp.qd.data(), d, b, &qp)) return rc;
  const size_t rnz = sp.rci.size();
  if (dalloc(h, &qp->r_rowptr, (size_t)n + 1) || dalloc(h, &qp->r_colind, rnz) || dalloc(h, &qp->r_vals, rnz) ||
      dalloc(h, &qp->d_eff, (size_t)n) || dalloc(h, &qp->tail, (size_t)n)) {
    delete qp;
    return FPSQ_ERR_HIP;
  }
  if (hipMemcpy(qp->r_rowptr, sp.rrp.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (rnz && (hipMemcpy(qp->r_colind, sp.rci.data(), rnz * 4, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(qp->r_vals, sp.rv.data(), rnz * 8, hipMemcpyHostToDevice) != hipSuccess))) {
    h->err = "qp_create_csr: cannot upload the objective Hessian";
    delete qp;
    return FPSQ_ERR_HIP;
  }
  qp->lgR = lane_group((int64_t)rnz, n);
  const int64_t tiles = std::max<int64_t>(1, (n + kBlock / qp->lgR - 1) / (kBlock / qp->lgR));
  qp->gridF = (int)std::min<int64_t>(tiles, kEwBlocksMax);      // (pQ holds 2 kEwBlocksMax partials: the start-up's, then these)
  qp->gridR = (int)std::min<int64_t>(tiles, 2 * kEwBlocksMax);  // (256 CUs x 8 resident workgroups of 256 threads)
  *out = qp;
  return FPSQ_OK;
}

}  // extern "C"

namespace {
// one launch of the row-product kernel on R of a model with a sparse objective Hessian
template <int MODE>
void launch_qp_csr(fpsq_handle h, fpsq_qp qp, const double* a, const double* b, const double* in, double* out, double* pf, double* pz,
                   Gates gates = Gates{}) {
  QrArgs A{qp->r_rowptr, qp->r_colind, qp->r_vals, a, b, in, out, pf, pz, (int32_t)h->n};
  const int grid = MODE == QR_FRONT ? qp->gridF : qp->gridR;
  WITH_LANE_GROUP(qp->lgR, hipLaunchKernelGGL((k_qp_csr<LG, MODE>), dim3(grid), dim3(kBlock), 0, h->stream, A, gates.c0, gates.c1));
  if (MODE != QR_HSV) h->launches++;  // (QR_HSV stands in for k_qp_hsv, which the epilogue of hprod counts)
}
}  // namespace

namespace {
// stand-alone form of qp_fx (sharded runs: the m-vector sums pass through an all-reduce first)
__global__ __launch_bounds__(kBlock) void k_qp_fx(const FxArgs a, const LaneCtl* gate0, const LaneCtl* gate1) {
  if (gate0 != nullptr && !(gate0->done && gate1->done)) return;
  __shared__ double red[kFxRed];
  qp_fx(a, red);
}
}  // namespace

extern "C" {

static int impl_qp_objgrad(fpsq_handle h, fpsq_qp qp, const double* x, double sigma, double rho, double eta,
                    const double* xk, double* fx, double* gx, double* ys, double* gs, fpsq_stats st[2]) {
  if (h && h->ab_dynamic)
    if (const char* ev = std::getenv("FPSQ_AB_MASK")) h->ab_mask = std::atoi(ev);
  if (h && h->host_trace) {
    const auto now = std::chrono::steady_clock::now();
    if (h->ht_have_exit) h->ht_sum[0] += std::chrono::duration<double>(now - h->ht_exit).count();
    h->ht_last = now;
    h->ht_calls++;
  }
  if (int rc = check_ready(h)) return rc;
  if (!qp || qp->h != h || !x || !st || (eta > 0.0 && !xk)) {
    h->err = "qp_objgrad: bad argument";
    return FPSQ_ERR_ARG;
  }
  const bool sparse_q = qp->r_rowptr != nullptr;  // Q = diag(q) + R (fpsq_qp_create_csr): two launches more, fpsq_qp_csr.hip.h
  if (sparse_q)
    if (int rc = sparse_q_scope(h, "qp_objgrad")) return rc;
  hipSetDevice(h->opt.device);
  hipStream_t s = h->stream;
  order_inputs(h);
  ht_mark(h, 1);
  const int64_t n = h->n, m = h->m;
  const size_t nb = (size_t)n * 8, mb = (size_t)m * 8;
  const int gn = ew_grid(n), gm = ew_grid(m);
  // x and gx resident on this GPU are used in place (no staging copy); host buffers go through h->xin / h->gx
  const double* dx = x;
  if (!on_this_device(h, x)) {
    HIPCHK(h, hipMemcpyAsync(h->xin, x, nb, hipMemcpyDefault, s));
    dx = h->xin;
  }
  double* dgx = gx && on_this_device(h, gx) ? gx : h->gx;
  const double* dxk = nullptr;
  if (eta > 0.0) {
    HIPCHK(h, hipMemcpyAsync(h->xk, xk, nb, hipMemcpyDefault, s));
    dxk = h->xk;
  }
  call_begin(h);
  // user-model evaluations of _compute_ys_gs!  (src/model-Fletcherpenaltynlp.jl:238-240)
  // Fast start (single GPU, fused recurrences): the gradient kernel writes the long pair {g, x} itself and the LSQR
  // start-up product A u~_1, in which the CRAIG lane is otherwise parked, forms c = A x - b on the side: the separate
  // c = A x - b product and the right-hand-side loads of the start-up are not launched.
  const bool local_vec = !h->comm || h->halo;  // single GPU, or row-sharded with column windows (halo mode)
  const bool fast = local_vec && h->opt.fuse_two_rhs != 0 && h->opt.kkt_method == FPSQ_KKT_LSQR_CRAIG;
  RunRequest req;
  // sparse Q, in front: d_eff = d + R x and the partials of -1/2 x'R x behind the gn partials of f (zeros behind those of
  // ||x - xk||^2): the gradient body below then forms g = q.*x + d_eff = Q x + d and sums f + 1/2 x'R x, unchanged
  const int gr = sparse_q ? qp->gridF : 0;
  if (sparse_q) launch_qp_csr<QR_FRONT>(h, qp, dx, nullptr, qp->d, qp->d_eff, h->pQ[0] + gn, h->pQ[1] + gn);
  double* tgx = sparse_q ? qp->tail : dgx;  // (the tail's gx: the gated launch behind it writes dgx = tgx - R p2)
  {
    QpGradArgs qg{qp->q, sparse_q ? qp->d_eff : qp->d, dx, dxk, h->g, n, h->pQ[0], h->pQ[1], fast ? h->LP : (double*)nullptr,
                  fast ? h->pE : (double*)nullptr, n_owned(h), gn};
    if (fast && !(h->ab_mask & 1)) {
      req.startup_qg = qg;  // evaluated by the start-up launch of the recurrences (k_startup): no launch of its own
    } else {
      hipLaunchKernelGGL(k_qp_grad, dim3(gn), dim3(kBlock), 0, s, qg);
      h->launches++;
    }
  }
  ht_mark(h, 2);
  if (!fast) spmv_const(h, TAG_A, 1.0, dx, -1.0, qp->b, h->c);  // c = A x - b
  // Single GPU with rho > 0: p1 = g - A'q1 and J'c (:424-428) share ONE two-right-hand-side product A'[q1, c], and
  // phi is reduced by an extra workgroup of the gradient kernel: 2 launches fewer at the end of every evaluation.
  // (halo mode: the same product, its overlap rows completed after the neighbour exchange; phi needs its all-reduce)
  const bool paired = local_vec && rho > 0.0;
  // the epilogue then starts with k_ys, which also applies the final LSQR x update (no launch of its own for it)
  req.absorb_flush = paired && fast && !(h->ab_mask & 2);
  const double seq = (h->call_seq += 1.0);
  // CRAIG without x in its loop: the one-launch tail forms v = p2 = -A'q2 on the side (else two_mixed_device does, ahead of the tail)
  // (FPSQ_FUSE_TAIL=0 too: there the plain raw product carries the same single-lane pass -- k_spmv<2, .., VRAW>)
  const bool v_in_tail = paired && craig_x_from_y(h) && h->AT.sorted && h->AT.padded && !h->craig_v_alone;
  // everything behind the two solves: enqueued speculatively (gated on the recurrences' `done` flags) by run_krylov when
  // the iteration count of the previous evaluation is known, else here
  TailFn epi = [&](const TailCtx& t) -> int {
    // ys = q1 + sigma q2 and the dots of objgrad!
    hipLaunchKernelGGL(k_ys, dim3(gm), dim3(kBlock), 0, s, h->Lx[0], h->Cy, h->c, sigma, h->ys, m, h->pC[0], h->pC[1],
                       paired ? h->SP : (double*)nullptr, t.gates.c0, t.gates.c1, t.flush);
    h->launches++;
    FxArgs fa{};
    fa.seq = seq;
    fa.pf = h->pQ[0];
    fa.pdx = h->pQ[1];
    fa.np_n = gn + gr;
    fa.pcy = h->pC[0];
    fa.pcc = h->pC[1];
    fa.np_m = gm;
    fa.rho = rho;
    fa.eta = eta;
    fa.out = h->hscal_dev;
    fa.stride = 1;
    // (row-sharded with in-launch sums: the reduction adds the ranks' four local sums up itself, in rank order -- xch_sum)
    const bool in_launch = insum(h);
    if (const XchTable* xt = in_launch ? insum_table(h) : nullptr) {
      fa.xt = xt;
      fa.xseq = next_xseq(h);
    }
    FxArgs none = fa;
    none.out = nullptr;
    if (paired) {
      // phi: by default the extra workgroup of the gradient kernel below.  FPSQ_AB_MASK & 4: a one-workgroup launch of its
      // own right behind k_ys (everything it sums is complete there), which puts the scalar on the host a whole product +
      // gradient kernel earlier for the stream-ordered return -- measured on one handle: 814.7 against 818.8 evals/s, the
      // extra launch costs more than the earlier return gains.  (Round 3 first let it ride in the product launch as its
      // first workgroup: the extra case in the product kernel's update switch cost the A' kernel 11 VGPRs and ~5 % of its
      // time -- 2 % of an evaluation.)
      const bool early_fx = in_launch && (h->ab_mask & 4);
      if (early_fx) {
        hipLaunchKernelGGL(k_qp_fx, dim3(1), dim3(kBlock), 0, s, fa, t.gates.c0, t.gates.c1);
        h->launches++;
      }
      const bool grad_fx = in_launch && !early_fx;
      // one GPU: the rows of the raw product go straight into grad(phi) -- one launch, and the 16 MB product is neither written nor
      // re-read (k_spmv<.., GRAD>; bitwise the two launches below, FPSQ_FUSE_TAIL=0)
      // (a communicator of ONE rank has no overlap rows and no peers: the single-GPU tail)
      bool one_launch = false;
      if (single_gpu_tail(h)) {
        GradEpi ge{};
        ge.g = h->g;
        ge.v = h->Cx;
        if (v_in_tail) {  // (v = p2 = kMixedXSign A'q2 is formed in this launch, from the final q2)
          ge.y2 = h->Cy;
          ge.vsign = kMixedXSign;
          ge.vout = h->Cx;
        }
        ge.q = qp->q;
        ge.x = dx;
        ge.xk = dxk;
        ge.sigma = sigma;
        ge.rho = rho;
        ge.eta = eta;
        ge.gs = h->gs;
        ge.gx = tgx;
        ge.fx = grad_fx ? fa : none;
        one_launch = launch_at_tail<2>(h, h->SP, h->LP, ge, t.gates);
      }
      if (!one_launch && v_in_tail) {  // (FPSQ_FUSE_TAIL=0: the plain raw product, with v on the side: k_spmv<2, .., VRAW>)
        GradEpi ge{};
        ge.y2 = h->Cy;
        ge.vsign = kMixedXSign;
        ge.vout = h->Cx;
        launch_at_tail<2, true>(h, h->SP, h->LP, ge, t.gates);
      } else if (!one_launch) {
        launch_spmv<2>(h, TAG_AT, h->SP, nullptr, h->LP, h->ctl_raw, h->ctl_raw, nullptr, seg_none(), seg_none(), h->halo, nullptr,
                       t.gates);
      }
      if (!one_launch) {  // (the product writes its rows as ever: combine them in a launch of their own)
        if (h->halo)
          if (int rc = halo_finish<2>(h, nullptr, h->LP, h->ctl_raw, h->ctl_raw, nullptr, t.gates)) return rc;
        hipLaunchKernelGGL(k_qp_penalty_grad, dim3(grad_fx ? gn + 1 : gn), dim3(kBlock), 0, s, (const double*)nullptr, h->g, h->LP,
                           h->Cx, qp->q, (const double*)nullptr, dx, dxk, sigma, rho, eta, h->gs, tgx, n, grad_fx ? fa : none,
                           t.gates.c0, t.gates.c1);
        h->launches++;
      }
    } else {
      if (rho > 0.0)
        if (int rc = at_product_const(h, 1.0, h->c, 0.0, nullptr, h->jc, t.gates)) return rc;  // J'c   (:424-428)
      hipLaunchKernelGGL(k_qp_penalty_grad, dim3(in_launch ? gn + 1 : gn), dim3(kBlock), 0, s, h->p1, h->g,
                         (const double*)nullptr, h->Cx, qp->q, h->jc, dx, dxk, sigma, rho, eta, h->gs, tgx, n,
                         in_launch ? fa : none, t.gates.c0, t.gates.c1);
      h->launches++;
    }
    // sparse Q, behind whichever tail ran (p2 = v is in h->Cx after each of them): gx = tgx - R p2, gated like the tail.  Out of
    // place, so an epilogue that is enqueued twice writes the same bytes twice
    if (sparse_q) launch_qp_csr<QR_SUB>(h, qp, h->Cx, nullptr, tgx, dgx, nullptr, nullptr, t.gates);
    if (!in_launch) {  // phi: c'ys and c'c are sums over the rank's rows only
      PresumArgs P{};
      P.p[0] = fa.pcy;
      P.n[0] = gm;
      P.p[1] = fa.pcc;
      P.n[1] = gm;
      if (h->halo) {  // f and ||x - xk||^2 are sums over the owned part of the rank's column window
        P.p[2] = fa.pf;
        P.n[2] = gn;
        P.p[3] = fa.pdx;
        P.n[3] = gn;
      }
      hipLaunchKernelGGL(k_presum, dim3(1), dim3(kBlock), 0, s, P, h->comm_scal);
      if (h->halo) {
        // the ranks' four local sums are ALL-GATHERED like the norm partials of the loop (through the same two buffers:
        // on the peer-to-peer route no collective call here either) and summed by every rank in rank order: phi is
        // bitwise the same on every rank whatever a reduction algorithm would do
        const int P_ = h->comm->nranks;
        double* gbuf = h->gath + (size_t)(h->gather_calls++ & 1) * (size_t)h->seg_len * P_;
        if (int rc = h->comm->allgather(h->comm_scal, gbuf, 4, s)) {
          h->err = h->comm->err;
          return rc;
        }
        fa.pcy = gbuf;
        fa.pcc = gbuf + 1;
        fa.pf = gbuf + 2;
        fa.pdx = gbuf + 3;
        fa.np_m = fa.np_n = P_;
        fa.stride = 4;
      } else {
        if (int rc = comm_allreduce(h, h->comm_scal, 4)) return rc;
        fa.pcy = h->comm_scal;
        fa.pcc = h->comm_scal + 1;
        fa.np_m = 1;
      }
      hipLaunchKernelGGL(k_qp_fx, dim3(1), dim3(kBlock), 0, s, fa, t.gates.c0, t.gates.c1);
      h->launches += 2;
    }
    return 0;
  };
  if (int rc = two_mixed_device(h, h->g, h->c, paired, fast ? qp->b : nullptr, local_vec ? &epi : nullptr, req, v_in_tail)) return rc;
  if (!local_vec)
    if (int rc = epi(TailCtx{})) return rc;
  if (gx && dgx != gx) HIPCHK(h, hipMemcpyAsync(gx, h->gx, nb, hipMemcpyDefault, s));
  if (ys) HIPCHK(h, hipMemcpyAsync(ys, h->ys, mb, hipMemcpyDefault, s));
  if (gs) HIPCHK(h, hipMemcpyAsync(gs, h->gs, nb, hipMemcpyDefault, s));
  ht_mark(h, 5);
  // Stream-ordered outputs (fpsq_set_output_ordering): with every vector argument resident on this GPU the call returns
  // once phi and the statistics are on the host; the registered stream is made to wait for the rest of the epilogue.
  const bool ordered = h->out_ordered && !(h->ab_mask & 8) && h->in_stream_on && !h->profile && insum(h) && paired && dx == x &&
                       (!gx || dgx == gx) && (!ys || on_this_device(h, ys)) && (!gs || on_this_device(h, gs));
  if (ordered) {
    if (int rc = call_end_ordered(h, seq)) return rc;
  } else {
    if (int rc = call_end(h)) return rc;
  }
  ht_mark(h, 6);
  if (fx) *fx = h->hscal[0];
  st[0] = h->hstats[0];
  st[1] = h->hstats[1];
  if (h->host_trace) {
    ht_mark(h, 7);
    h->ht_exit = h->ht_last;
    h->ht_have_exit = true;
  }
  return soft_rc(st);
}

static int impl_qp_hprod(fpsq_handle h, fpsq_qp qp, const double* v, double sigma, double rho, double eta,
                  int32_t hessian_approx, double* Hv, fpsq_stats* st) {
  if (int rc = check_ready(h)) return rc;
  if (!qp || qp->h != h || !v || !Hv || !st || (hessian_approx != 1 && hessian_approx != 2)) {
    h->err = "qp_hprod: bad argument (hessian_approx is 1 or 2)";
    return FPSQ_ERR_ARG;
  }
  const bool sparse_q = qp->r_rowptr != nullptr;  // Q = diag(q) + R (fpsq_qp_create_csr): one launch more, fpsq_qp_csr.hip.h
  if (sparse_q)
    if (int rc = sparse_q_scope(h, "qp_hprod")) return rc;
  hipSetDevice(h->opt.device);
  hipStream_t s = h->stream;
  order_inputs(h);
  const int64_t n = h->n;
  const size_t nb = (size_t)n * 8;
  const int gn = ew_grid(n);
  const double* dv = v;
  if (!on_this_device(h, v)) {
    HIPCHK(h, hipMemcpyAsync(h->in_n1, v, nb, hipMemcpyDefault, s));
    dv = h->in_n1;
  }
  double* dhv = on_this_device(h, Hv) ? Hv : h->gx;
  bool lsq_repeats = false;
  call_begin(h);
  double* thv = sparse_q ? qp->tail : dhv;  // (the tail's Hv: the gated launch behind it writes dhv = thv - R (v - p1))
  if (sparse_q) {
    launch_qp_csr<QR_HSV>(h, qp, dv, nullptr, qp->q, h->in_n2, nullptr, nullptr);  // Hsv = q .* v + R v = Q v            :537
  } else {
    hipLaunchKernelGGL(k_qp_hsv, dim3(gn), dim3(kBlock), 0, s, qp->q, dv, h->in_n2, n);                  // :537
  }
  TailFn epi = [&](const TailCtx& t) -> int {
    bool fin_done = false;
    if (rho > 0.0) {                                                                                      // :557-558
      spmv_const(h, TAG_A, 1.0, dv, 0.0, nullptr, h->in_m, t.gates);
      // one GPU: the rows of A'(A v) go straight into Hv (k_spmv<1, .., GRAD>; bitwise the product + k_qp_hprod_fin, FPSQ_FUSE_TAIL=0)
      if (single_gpu_tail(h)) {
        GradEpi ge{};
        ge.p1 = h->p1;
        ge.p2 = h->p2b;
        ge.v = dv;
        ge.q = qp->q;
        ge.sigma = sigma;
        ge.rho = rho;
        ge.eta = eta;
        ge.hv = thv;
        fin_done = launch_at_tail<1>(h, h->in_m, h->jc, ge, t.gates);
      }
      if (!fin_done)
        if (int rc = at_product_const(h, 1.0, h->in_m, 0.0, nullptr, h->jc, t.gates)) return rc;
    }
    if (!fin_done) {
      hipLaunchKernelGGL(k_qp_hprod_fin, dim3(gn), dim3(kBlock), 0, s, h->p1, h->p2b, qp->q, dv, h->jc, sigma, rho, eta, thv,
                         n, t.gates.c0, t.gates.c1);                                                      // :543-562
      h->launches++;
    }
    h->launches++;
    // sparse Q: Hv = thv - R (v - p1), gated like the tail and out of place like objgrad's
    if (sparse_q) launch_qp_csr<QR_SUB>(h, qp, dv, h->p1, thv, dhv, nullptr, nullptr, t.gates);
    return 0;
  };
  const bool local_vec = !h->comm || h->halo;
  if (int rc = two_least_squares_device(h, dv, h->in_n2, local_vec ? &epi : nullptr)) return rc;         // :542
  if (!local_vec)
    if (int rc = epi(TailCtx{})) return rc;
  if (hessian_approx == 1) {
    // Val(1) (src/model-Fletcherpenaltynlp.jl:572-634) adds, on top of everything above:
    //   Ssv = ghjvprod(x, gs, v) = 0 (linear constraints);  (invJtJJv, invJtJSsv) = solve_two_extras(v, Ssv)   :601-602
    //   Hv -= J' invJtJSsv                                                                                  :603-611
    //   Hv -= hprod_nln(x, invJtJJv, gs; obj_weight = 0) = 0                                                :613-614
    // i.e. the LSQR + MINRES lanes of solve_two_extras (tau = max(delta, 1e-14)) on the right-hand sides (v, 0) and one
    // more A' product; the two recurrences' statistics go to st[2], st[3].
    // For this model two of those pieces are known in advance (FPSQ_AB_MASK bit 16 computes them all the same, for the test
    // that holds the results bitwise equal): the MINRES lane's right-hand side is zero, so its solution is zero and so is
    // J' invJtJSsv -- no A' product, nothing to subtract; and when tau == delta (delta >= 1e-14) the LSQR lane repeats, bit
    // for bit, the first solve of solve_two_least_squares above (solve_least_square on the same operator, right-hand side v
    // and damping: linear_system.jl:53 against :87) -- its statistics are that solve's.
    const double tau = std::max(h->delta, 1e-14);
    const bool full = (h->ab_mask & 16) != 0;
    lsq_repeats = !full && tau == h->delta;
    HIPCHK(h, hipMemsetAsync(h->in_m, 0, (size_t)h->m * 8, s));
    Lane lanes[2];
    lanes[0].kind = LANE_LSQR;
    lanes[0].rhs = dv;
    lanes[0].lambda = std::sqrt(tau);
    lanes[0].x = h->Lx[0];
    lanes[0].st = &h->hstats[2];
    lanes[1].kind = LANE_MINRES;
    lanes[1].rhs = h->in_m;
    lanes[1].lambda = tau;
    lanes[1].x = h->Mx;
    lanes[1].st = &h->hstats[3];
    if (lsq_repeats) {
      if (int rc = run_lanes(h, lanes + 1, 1)) return rc;
    } else {
      if (int rc = run_lanes(h, lanes, 2)) return rc;
    }
    if (full) {
      if (int rc = at_product_const(h, 1.0, h->Mx, 0.0, nullptr, h->jc)) return rc;  // J' invJtJSsv
      hipLaunchKernelGGL(k_axpby_plain, dim3(gn), dim3(kBlock), 0, s, h->jc, -1.0, dhv, 1.0, dhv, n);
      h->launches++;
    }
  }
  if (dhv != Hv) HIPCHK(h, hipMemcpyAsync(Hv, dhv, nb, hipMemcpyDefault, s));
  if (int rc = call_end(h)) return rc;
  st[0] = h->hstats[0];
  st[1] = h->hstats[1];
  int rc = soft_rc(st);
  if (hessian_approx == 1) {
    st[2] = lsq_repeats ? h->hstats[0] : h->hstats[2];
    st[3] = h->hstats[3];
    rc |= soft_rc(st + 2) << 2;
  }
  return rc;
}

int fpsq_comm_unique_id(uint8_t id[128]) {
  std::string err;
  if (!id || !g_rccl.load(err)) {
    g_create_error = err.empty() ? "comm_unique_id: null argument" : err;
    return FPSQ_ERR_COMM;
  }
  ncclUniqueId u;
  ncclResult_t r = g_rccl.GetUniqueId(&u);
  if (r != ncclSuccess) {
    g_create_error = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r);
    return FPSQ_ERR_COMM;
  }
  static_assert(sizeof(u) == 128, "ncclUniqueId is 128 bytes");
  std::memcpy(id, &u, 128);
  return FPSQ_OK;
}

int fpsq_comm_init(fpsq_handle h, int32_t nranks, int32_t rank, const uint8_t id[128]) {
  if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks || h->comm) {
    if (h) h->err = "comm_init: bad arguments or communicator already set";
    return FPSQ_ERR_ARG;
  }
  if (!g_rccl.load(h->err)) return FPSQ_ERR_COMM;
  hipSetDevice(h->opt.device);
  ncclUniqueId u;
  std::memcpy(&u, id, 128);
  IpcComm* c = new IpcComm();
  c->nranks = nranks;
  c->rank = rank;
  if (const char* ev = std::getenv("FPSQ_COMM_ROUTE"))  // rccl | p2p | auto (developer A/B; fpsq_comm_set_route is the API)
    c->want = !std::strcmp(ev, "rccl") ? FPSQ_ROUTE_RCCL : !std::strcmp(ev, "p2p") ? FPSQ_ROUTE_P2P : FPSQ_ROUTE_AUTO;
  ncclResult_t r = g_rccl.CommInitRank(&c->c, nranks, u, rank);
  if (r != ncclSuccess) {
    h->err = std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r);
    c->c = nullptr;
    delete c;
    return FPSQ_ERR_COMM;
  }
  if (c->nranks > 1) unadopt_stream(h);  // (a sharded handle keeps a stream of its own: its peers' launches must not queue behind the caller's work)
  h->comm = c;
  h->info.comm_route = c->route();
  return FPSQ_OK;
}

int fpsq_comm_set_route(fpsq_handle h, int32_t route) {
  IpcComm* c = h ? dynamic_cast<IpcComm*>(h->comm) : nullptr;
  if (!c || (route != FPSQ_ROUTE_AUTO && route != FPSQ_ROUTE_RCCL && route != FPSQ_ROUTE_P2P)) {
    if (h) h->err = "comm_set_route: needs the communicator of fpsq_comm_init; route is FPSQ_ROUTE_AUTO / _RCCL / _P2P";
    return FPSQ_ERR_ARG;
  }
  if (h->halo || h->gather_ready) {
    h->err = "comm_set_route: call before fpsq_comm_set_halo (the exchange buffers are allocated for the route)";
    return FPSQ_ERR_STATE;
  }
  c->want = route;
  return FPSQ_OK;
}

int fpsq_local_group_create(int32_t nshards, void** out) {
  if (!out || nshards < 1 || nshards > 8) return FPSQ_ERR_ARG;
  LocalGroup* g = new LocalGroup();
  g->n = nshards;
  for (int r = 0; r < nshards; ++r) {
    hipEventCreateWithFlags(&g->ready[r], hipEventDisableTiming);
    hipEventCreateWithFlags(&g->copied[r], hipEventDisableTiming);
  }
  hipEventCreateWithFlags(&g->done, hipEventDisableTiming);
  *out = g;
  return FPSQ_OK;
}

int fpsq_local_group_destroy(void* group) {
  LocalGroup* g = (LocalGroup*)group;
  if (!g) return FPSQ_ERR_ARG;
  for (int r = 0; r < g->n; ++r) {
    hipEventDestroy(g->ready[r]);
    hipEventDestroy(g->copied[r]);
  }
  hipEventDestroy(g->done);
  delete g;
  return FPSQ_OK;
}

int fpsq_local_group_set_p2p(void* group, int32_t on) {
  LocalGroup* g = (LocalGroup*)group;
  if (!g) return FPSQ_ERR_ARG;
  g->p2p = on != 0;
  return FPSQ_OK;
}

int fpsq_comm_init_local(fpsq_handle h, void* group, int32_t shard) {
  LocalGroup* g = (LocalGroup*)group;
  if (!h || !g || shard < 0 || shard >= g->n || h->comm) {
    if (h) h->err = "comm_init_local: bad arguments or communicator already set";
    return FPSQ_ERR_ARG;
  }
  LocalComm* c = g->p2p ? new P2PLocalComm() : new LocalComm();
  c->nranks = g->n;
  c->rank = shard;
  c->g = g;
  if (c->nranks > 1) unadopt_stream(h);  // (a sharded handle keeps a stream of its own: its peers' launches must not queue behind the caller's work)
  h->comm = c;
  h->info.comm_route = c->route();
  return FPSQ_OK;
}

int fpsq_comm_set_halo(fpsq_handle h, int64_t overlap_left, int64_t overlap_right) {
  if (!h || !h->comm || overlap_left < 0 || overlap_right < 0 || overlap_left + overlap_right > h->n ||
      (h->comm->rank == 0 && overlap_left != 0) || (h->comm->rank == h->comm->nranks - 1 && overlap_right != 0)) {
    if (h) h->err = "comm_set_halo: needs a communicator; overlaps must fit the window and vanish at the outer ends";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(h->opt.device);
  if (h->gather_ready) {
    h->err = "comm_set_halo: call before the first solve";
    return FPSQ_ERR_STATE;
  }
  if (h->halo_recv) dfree(h, &h->halo_recv);
  if (h->halo_raw) dfree(h, &h->halo_raw);
  if (int rc = xalloc(h, &h->halo_recv, (size_t)(overlap_left + overlap_right) * 2 * 2)) return rc;
  if (int rc = dalloc(h, &h->halo_raw, (size_t)(overlap_left + overlap_right) * 2)) return rc;
  h->halo_gf = overlap_left + overlap_right > 0 ? ew_grid(overlap_left + overlap_right) : 0;
  h->halo = true;
  h->ovl = overlap_left;
  h->ovr = overlap_right;
  if (h->have_structure)
    if (int rc = setup_fused_halo(h)) return rc;
  return FPSQ_OK;
}

int fpsq_get_info(fpsq_handle h, fpsq_info* info) {
  if (!h || !info) return FPSQ_ERR_ARG;
  *info = h->info;
  return FPSQ_OK;
}

int fpsq_debug_expect_iterations(fpsq_handle h, int64_t expect) {
  if (!h) return FPSQ_ERR_ARG;
  h->force_expect = expect;
  return FPSQ_OK;
}

int fpsq_set_profiling(fpsq_handle h, int32_t on) {
  if (!h) return FPSQ_ERR_ARG;
  h->profile = on != 0;
  return FPSQ_OK;
}

// the solve entries, each repeated once on two launches per iteration when a one-launch iteration ran into a bounded wait
int fpsq_solve_two_mixed(fpsq_handle h, const double* rhs1, const double* rhs2, double* p1, double* q1, double* p2,
                         double* q2, fpsq_stats st[2]) {
  return with_fuse_fallback(h, [&]() { return impl_solve_two_mixed(h, rhs1, rhs2, p1, q1, p2, q2, st); });
}
int fpsq_solve_two_least_squares(fpsq_handle h, const double* rhs1, const double* rhs2, double* p1, double* q1,
                                 double* p2, double* q2, fpsq_stats st[2]) {
  return with_fuse_fallback(h, [&]() { return impl_solve_two_least_squares(h, rhs1, rhs2, p1, q1, p2, q2, st); });
}
int fpsq_solve_two_extras(fpsq_handle h, const double* rhs1, const double* rhs2, double* out1, double* out2,
                          fpsq_stats st[2]) {
  return with_fuse_fallback(h, [&]() { return impl_solve_two_extras(h, rhs1, rhs2, out1, out2, st); });
}
int fpsq_qp_objgrad(fpsq_handle h, fpsq_qp qp, const double* x, double sigma, double rho, double eta,
                    const double* xk, double* fx, double* gx, double* ys, double* gs, fpsq_stats st[2]) {
  return with_fuse_fallback(h, [&]() { return impl_qp_objgrad(h, qp, x, sigma, rho, eta, xk, fx, gx, ys, gs, st); });
}
int fpsq_qp_hprod(fpsq_handle h, fpsq_qp qp, const double* v, double sigma, double rho, double eta,
                  int32_t hessian_approx, double* Hv, fpsq_stats* st) {
  return with_fuse_fallback(h, [&]() { return impl_qp_hprod(h, qp, v, sigma, rho, eta, hessian_approx, Hv, st); });
}
}  // extern "C"
