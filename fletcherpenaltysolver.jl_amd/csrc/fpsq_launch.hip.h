// fpsq_launch.hip.h -- launch helpers of the products and the sums behind them: ht_mark, launch_product, Gates, launch_spmv,
// launch_at_tail / launch_at_seam, spmv_const, comm_allreduce, halo_finish, at_product*, wait_progress.
// Part of fpsq.hip's translation unit.
#pragma once

#include "fpsq_structure.hip.h"

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>

namespace {

// ------------------------------------------------------------------ launch helpers

inline void ht_mark(fpsq_handle h, int k) {
  if (!h->host_trace) return;
  const auto now = std::chrono::steady_clock::now();
  h->ht_sum[k] += std::chrono::duration<double>(now - h->ht_last).count();
  h->ht_last = now;
}


enum { TAG_A = 0, TAG_AT = 1 };

// Profiled product launches attach the event pair to the dispatch itself (hipExtLaunchKernelGGL): the elapsed time
// is the kernel's own start-to-end time, as rocprofv3 reports it.  Two hipEventRecord markers around the launch add
// ~5 us of marker processing to every sample.
template <typename K, typename... Args>
void launch_product(fpsq_handle h, K kernel, dim3 grid, Args... args) {
  if (!h->profile) {
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, h->stream, args...);
    return;
  }
  if (h->ev_used == h->ev_pool.size()) {
    EventPair p;
    hipEventCreate(&p.a);
    hipEventCreate(&p.b);
    h->ev_pool.push_back(p);
  }
  EventPair& e = h->ev_pool[h->ev_used++];
  hipExtLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, h->stream, e.a, e.b, 0, args...);
}

UpdSeg seg_none() {
  UpdSeg s{};
  s.kind = UPD_NONE;
  s.nblk = 0;
  return s;
}

GradEpi grad_none() { return GradEpi{}; }

// Speculative epilogue (run_krylov): kernels launched with gates only act once BOTH lane controls say `done` (none: always)
struct Gates {
  const LaneCtl* c0 = nullptr;
  const LaneCtl* c1 = nullptr;
};

// u0/u1: vector-update segments that ride in the product launch (run_fused_updates); they may only read what the
// product reads.
// halo_rows (A' products of a halo-mode handle): the overlap rows of the rank's column window only get their raw sums,
// see HaloRows / halo_finish.
// pre (two entries): the scalar steps of the two lanes that follow the previous product ride in this launch, with leader
// workgroups (k_spmv_atl / k_spmv_rgcs<.., LEAD>; run_krylov only hands steps over where both products have those variants)
template <int NL>
void launch_spmv(fpsq_handle h, int tag, const double* x, const double* yin, double* yout, const LaneCtl* c0,
                 const LaneCtl* c1, double* partials, const UpdSeg& u0 = seg_none(), const UpdSeg& u1 = seg_none(),
                 bool halo_rows = false, const StepArgs* pre = nullptr, Gates gates = {}) {
  const int nupd = u0.nblk + u1.nblk;
  const HaloRows hr{h->ovl, h->n - h->ovr, h->halo_raw};
  StepArgs z0{}, z1{};
  if (pre) {
    z0 = pre[0];
    z1 = pre[1];
  }
  RideArgs ra{};
  const bool lead = pre != nullptr;
  if (lead) {
    ra.rec = h->ride_rec;
    ra.want = (unsigned int)++h->ride_seq;
    ra.pub = h->ride_break ? ~ra.want : ra.want;
    ra.err = reinterpret_cast<unsigned long long*>(h->hscal_dev + 15);
    ra.delay = h->ride_delay;
    ra.xseq = h->ride_xseq;
    ra.xt = h->ride_xseq ? insum_table(h) : nullptr;
    ra.more = ra.xt ? h->comm->wait_more() : 0;  // (the leaders may be waiting for a late peer: whoever waits for them outlasts that)
  }
  if (tag == TAG_A && h->RA.ok) {
    const int per_xcd = (h->RA.view.ng + 7) / 8;
#define FPSQ_LAUNCH_RGCS(...) \
    launch_product(h, k_spmv_rgcs<__VA_ARGS__>, dim3(per_xcd * 8 + nupd + (lead ? kRideCand : 0)), h->RA.view, x, yin, yout, c0, c1, partials, \
                   per_xcd, u0, u1, gates.c0, gates.c1, h->strA, z0, z1, ra)
    if constexpr (NL == 2) {
      // (a sharded handle whose leaders form their sums over the ranks in the launch: the variants with the exchange compiled in)
      if (lead && ra.xt != nullptr && h->RA.view.stride) FPSQ_LAUNCH_RGCS(2, true, true, true);
      else if (lead && ra.xt != nullptr) FPSQ_LAUNCH_RGCS(2, false, true, true);
      else if (lead && h->RA.view.stride) FPSQ_LAUNCH_RGCS(2, true, true);
      else if (lead) FPSQ_LAUNCH_RGCS(2, false, true);
    }
    if (!pre) {
      if (h->RA.view.stride) FPSQ_LAUNCH_RGCS(NL, true);
      else FPSQ_LAUNCH_RGCS(NL, false);
    }
#undef FPSQ_LAUNCH_RGCS
  } else {
    const DevCsr& M = tag == TAG_A ? h->A : h->AT;
    const int per_xcd = (M.nblk + 7) / 8;
    const dim3 grid(per_xcd * 8 + nupd);
    const int ps = tag == TAG_A ? h->strA : h->strT;
#define FPSQ_LAUNCH_SPMV(...) \
    launch_product(h, k_spmv<__VA_ARGS__>, grid, M.view(), x, yin, yout, c0, c1, partials, per_xcd, u0, u1, gates.c0, gates.c1, ps, hr, \
                   grad_none())
    bool done_pre = false;
    if constexpr (NL == 2) {
      if (lead) {  // (tag == TAG_AT: padded blocks with block-relative columns)
        done_pre = true;
        // the first resident set of workgroups takes two row blocks each (see k_spmv_atl)
        const int R = h->resident_wgs - kRideCand;
        int n2 = !h->atl_two || M.nblk <= R ? 0 : std::min(R, M.nblk - R);
        int nwg = M.nblk - n2;
        int bpx = 0;
        if (h->at_xcd) {  // XCD-contiguous eighths of the row blocks (FPSQ_AT_XCD=0: grid order)
          bpx = (M.nblk + 7) / 8;
          const int n2e = std::min(n2 / 8, bpx / 2);
          n2 = 8 * n2e;
          nwg = 8 * (bpx - n2e);
        }
        const dim3 lgrid(kRideCand + nwg + nupd);
        if (M.sorted && halo_rows)
          launch_product(h, k_spmv_atl<true, true>, lgrid, M.view(), x, yin, yout, partials, nwg, n2, u0, u1, ps, z0, z1, ra, hr, bpx);
        else if (M.sorted)
          launch_product(h, k_spmv_atl<true, false>, lgrid, M.view(), x, yin, yout, partials, nwg, n2, u0, u1, ps, z0, z1, ra, hr, bpx);
        else if (halo_rows)
          launch_product(h, k_spmv_atl<false, true>, lgrid, M.view(), x, yin, yout, partials, nwg, n2, u0, u1, ps, z0, z1, ra, hr, bpx);
        else
          launch_product(h, k_spmv_atl<false, false>, lgrid, M.view(), x, yin, yout, partials, nwg, n2, u0, u1, ps, z0, z1, ra, hr, bpx);
      }
    }
    if (done_pre) {
    } else if (tag == TAG_A && M.col16) FPSQ_LAUNCH_SPMV(NL, TAG_A, true);
    else if (tag == TAG_A) FPSQ_LAUNCH_SPMV(NL, TAG_A, false);
    else if (halo_rows) {
      if (M.sorted) FPSQ_LAUNCH_SPMV(NL, TAG_AT, true, true, true, true);
      else if (M.col16 && M.padded) FPSQ_LAUNCH_SPMV(NL, TAG_AT, true, true, true);
      else if (M.col16) FPSQ_LAUNCH_SPMV(NL, TAG_AT, true, false, true);
      else if (M.padded) FPSQ_LAUNCH_SPMV(NL, TAG_AT, false, true, true);
      else FPSQ_LAUNCH_SPMV(NL, TAG_AT, false, false, true);
    } else if (M.sorted) FPSQ_LAUNCH_SPMV(NL, TAG_AT, true, true, false, true);
    else if (M.col16 && M.padded) FPSQ_LAUNCH_SPMV(NL, TAG_AT, true, true);
    else if (M.col16) FPSQ_LAUNCH_SPMV(NL, TAG_AT, true);
    else if (M.padded) FPSQ_LAUNCH_SPMV(NL, TAG_AT, false, true);
    else FPSQ_LAUNCH_SPMV(NL, TAG_AT, false);
#undef FPSQ_LAUNCH_SPMV
  }
  h->launches++;
  h->spmv_launches++;
  (tag == TAG_A ? h->prod_a : h->prod_at)[NL - 1]++;
}

// The tail of a call runs as on one GPU: no communicator, or one of ONE rank (no overlap rows, no peers: its products need no
// sum over the ranks), and an A' layout with a GRAD variant
inline bool single_gpu_tail(fpsq_handle h) {
  return h->fuse_tail && (!h->comm || (h->comm->nranks == 1 && h->ovl + h->ovr == 0)) && h->AT.sorted && h->AT.padded;
}

// The tail's raw A' product on one GPU: its rows go straight into the call's result (k_spmv<.., GRAD>; grad(phi): two lanes,
// Hv: one).  False: the layout has no GRAD variant, nothing was launched (the caller launches the product and the kernel that
// combines its rows).
// VRAW (two lanes, FPSQ_FUSE_TAIL=0): the rows ARE written, as launch_spmv<2> writes them, and v = ge.vsign A'ge.y2 goes to ge.vout
// beside them (nothing else of `ge` is used).
template <int NL, bool VRAW = false>
bool launch_at_tail(fpsq_handle h, const double* x, double* yout, const GradEpi& ge, Gates gates = {}) {
  const DevCsr& M = h->AT;
  if (!M.sorted) return false;
  const int per_xcd = (M.nblk + 7) / 8;
  const HaloRows hr{h->ovl, h->n - h->ovr, h->halo_raw};
  if constexpr (VRAW)
    launch_product(h, k_spmv<NL, TAG_AT, true, true, false, true, false, true>, dim3(per_xcd * 8), M.view(),
                   x, (const double*)nullptr, yout, h->ctl_raw, h->ctl_raw, (double*)nullptr, per_xcd,
                   seg_none(), seg_none(), gates.c0, gates.c1, h->strT, hr, ge);
  else
  launch_product(h, k_spmv<NL, TAG_AT, true, true, false, true, true>, dim3(per_xcd * 8 + (ge.fx.out != nullptr ? 1 : 0)), M.view(),
                 x, (const double*)nullptr, yout, h->ctl_raw, h->ctl_raw, (double*)nullptr, per_xcd,
                 seg_none(), seg_none(), gates.c0, gates.c1, h->strT, hr, ge);
  h->launches++;
  h->spmv_launches++;
  h->prod_at[NL - 1]++;
  return true;
}

// p1 = g - A'q1 and v = vsign A'q2 of two plain vectors in ONE launch (k_spmv_seam): what fpsq_solve_two_mixed and fpsq_ys_gs
// hand out behind the recurrences, bitwise the two single-lane products (at_product_const) it stands for
void launch_at_seam(fpsq_handle h, const double* q1, const double* g, double* p1, const double* q2, double vsign, double* v,
                    Gates gates = {}) {
  const DevCsr& M = h->AT;
  launch_product(h, k_spmv_seam, dim3((M.nblk + 7) / 8 * 8), M.view(), q1, q2, g, p1, vsign, v, gates.c0, gates.c1);
  h->launches++;
  h->spmv_launches++;
  h->prod_at[1]++;
}

__global__ void k_set_ctl(LaneCtl* c, double ca, double cb) {
  c->ca = ca;
  c->cb = cb;
  c->done = 0;
  c->skip = 0;
  c->upd_iter = -1;
}

// control block holding the host-given coefficient pair (ca, cb)
const LaneCtl* const_ctl(fpsq_handle h, double ca, double cb) {
  // the coefficient pairs of the hot path are resident constants: no set-up launch
  if (ca == 1.0 && cb == 0.0) return h->ctl_raw;
  if (ca == 1.0 && cb == -1.0) return h->ctl_pm;
  if (ca == -1.0 && cb == 1.0) return h->ctl_mp;
  if (ca == -1.0 && cb == 0.0) return h->ctl_m0;
  hipLaunchKernelGGL(k_set_ctl, dim3(1), dim3(1), 0, h->stream, h->ctl_tmp, ca, cb);
  h->launches++;
  return h->ctl_tmp;
}

// out = ca * op(A) x + cb * yin with host-given constants
void spmv_const(fpsq_handle h, int tag, double ca, const double* x, double cb, const double* yin, double* yout,
                Gates gates = {}) {
  const LaneCtl* c = const_ctl(h, ca, cb);
  launch_spmv<1>(h, tag, x, yin, yout, c, c, nullptr, seg_none(), seg_none(), false, nullptr, gates);
}

int comm_allreduce(fpsq_handle h, double* buf, size_t count) {
  if (int rc = h->comm->allreduce_sum(buf, count, h->stream)) {
    h->err = h->comm->err;
    return rc;
  }
  return 0;
}

// Sum over the ranks of the raw partial A' products in buf ([n][NL]): all-reduce of the replicated n-vector (the
// replicated layout; halo mode never comes here: see halo_finish)
int comm_reduce_long(fpsq_handle h, double* buf, int NL) { return comm_allreduce(h, buf, (size_t)h->n * NL); }

// LP <- ca A' SP + cb LP with norm partials (count returned in *np).  Sharded: every rank holds a row block A_r, so
// A'x = sum_r A_r' x_r: raw partial product -> all-reduce -> fused axpby + norm on the replicated result.
// Halo mode, after k_spmv<.., HALO>: exchange the raw sums of the two overlap regions with the neighbours, then finish
// those rows (yout = ca (own + neighbour's) + cb yin, squared-norm partials of the owned head region behind the product's).
template <int NL>
int halo_finish(fpsq_handle h, const double* yin, double* yout, const LaneCtl* c0, const LaneCtl* c1, double* partials,
                Gates gates = {}) {
  const int64_t t = h->ovl + h->ovr;
  if (t == 0) return 0;
  double* rl = h->halo_recv + (size_t)(h->halo_calls++ & 1) * (size_t)t * 2;
  {  // peer-to-peer routes: exchange + finish in one launch
    const HaloFinishArgs fa{h->halo_raw, rl, h->ovl, h->ovr, h->n - h->ovr, yin, yout, c0, c1,
                            partials ? partials + h->AT.nblk : nullptr, h->strT, 0 /* dbg: the route's */, gates.c0, gates.c1};
    if (h->comm->halo_exchange_finish(NL, fa, h->halo_gf, h->stream)) {
      h->launches++;
      return 0;
    }
  }
  if (int rc = h->comm->halo_exchange(h->halo_raw, t, NL, h->ovl, h->ovr, rl, rl + (size_t)h->ovl * NL, h->stream)) {
    h->err = h->comm->err;
    return rc;
  }
  hipLaunchKernelGGL(k_halo_finish<NL>, dim3(h->halo_gf), dim3(kBlock), 0, h->stream, h->halo_raw, rl, h->ovl,
                     h->ovr, h->n - h->ovr, yin, yout, c0, c1, partials ? partials + h->AT.nblk : nullptr, h->strT, gates.c0,
                     gates.c1);
  h->launches++;
  return 0;
}

template <int NL>
int at_product(fpsq_handle h, const double* x, double* y, const LaneCtl* c0, const LaneCtl* c1, double* partials,
               int* np, const UpdSeg& u0 = seg_none(), const UpdSeg& u1 = seg_none(), const StepArgs* pre = nullptr,
               Gates gates = {}) {
  if (!h->comm) {
    launch_spmv<NL>(h, TAG_AT, x, y, y, c0, c1, partials, u0, u1, false, pre, gates);
    *np = h->AT.nblk;
    return 0;
  }
  if (h->halo) {
    // every row the rank alone contributes to is finished by the product kernel exactly as on one GPU (so the vector
    // updates may ride in the launch); only the overlap rows wait for the neighbours
    launch_spmv<NL>(h, TAG_AT, x, y, y, c0, c1, partials, u0, u1, /*halo_rows=*/true, pre, gates);
    // (steps riding in that launch: the control blocks k_halo_finish must read are the ones the leaders have just written)
    const LaneCtl* f0 = pre ? reinterpret_cast<const LaneCtl*>(pre[0].state_out) : c0;
    const LaneCtl* f1 = pre ? reinterpret_cast<const LaneCtl*>(pre[NL - 1].state_out) : c1;
    if (int rc = halo_finish<NL>(h, y, y, f0, f1, partials, gates)) return rc;
    *np = h->AT.nblk + h->halo_gf;
    return 0;
  }
  launch_spmv<NL>(h, TAG_AT, x, nullptr, h->comm_vec, h->ctl_raw, h->ctl_raw, nullptr, seg_none(), seg_none(), false, nullptr, gates);
  if (int rc = comm_reduce_long(h, h->comm_vec, NL)) return rc;
  const int g = ew_grid(h->n);
  h->strT = g;  // replicated layout: the norm partials of the A' product come from this kernel, g per lane
  hipLaunchKernelGGL(k_axpby_norm<NL>, dim3(g), dim3(kBlock), 0, h->stream, h->comm_vec, y, c0, c1, h->n, n_owned(h),
                     partials);
  h->launches++;
  *np = g;
  return 0;
}

// out = ca A' x + cb yin (plain vectors, host constants), all-reduced when sharded
int at_product_const(fpsq_handle h, double ca, const double* x, double cb, const double* yin, double* yout,
                     Gates gates = {}) {
  if (!h->comm) {
    spmv_const(h, TAG_AT, ca, x, cb, yin, yout, gates);
    return 0;
  }
  if (h->halo) {
    const LaneCtl* c = const_ctl(h, ca, cb);
    launch_spmv<1>(h, TAG_AT, x, yin, yout, c, c, nullptr, seg_none(), seg_none(), /*halo_rows=*/true, nullptr, gates);
    return halo_finish<1>(h, yin, yout, c, c, nullptr, gates);
  }
  launch_spmv<1>(h, TAG_AT, x, nullptr, h->comm_vec, h->ctl_raw, h->ctl_raw, nullptr, seg_none(), seg_none(), false, nullptr, gates);
  if (int rc = comm_reduce_long(h, h->comm_vec, 1)) return rc;
  hipLaunchKernelGGL(k_axpby_plain, dim3(ew_grid(h->n)), dim3(kBlock), 0, h->stream, h->comm_vec, ca, yin, cb, yout, h->n);
  h->launches++;
  return 0;
}

// Bounded wait until the device has reached `target` iterations (or finished).  The progress word lives in
// host-mapped memory and is stored by the scalar kernels; if the stream drains without the word moving (which
// would mean the mapped store is not visible) we fall back to reading the device state explicitly.
// one consistent snapshot {iter, done} of a lane's progress word (a single 8-byte load: see publish())
inline Progress load_progress(const Progress* p) {
  const uint64_t v = *reinterpret_cast<const volatile uint64_t*>(p);
  Progress r;
  r.iter = (int32_t)(uint32_t)(v & 0xffffffffu);
  r.done = (int32_t)(uint32_t)(v >> 32);
  return r;
}

int wait_progress(fpsq_handle h, int lane, int target, const int32_t* dev_done, const int32_t* dev_iter) {
  Progress* p = &h->prog_host[lane];
  const auto t0 = std::chrono::steady_clock::now();
  int spins = 0;
  auto reached = [&]() {
    const Progress s = load_progress(p);
    return s.done || s.iter >= target;
  };
  while (!reached()) {
    if ((++spins & 63) == 0) {
      // a bounded wait inside a launch has expired (the handle's error word): nothing later in this call can be right, and the
      // recurrences' progress words will not move any more -- leave the loop now, not at itmax (advisor, round 4)
      // (stop WAITING, not the call: the end of the call reads the word, switches the handle to two launches per iteration and has
      // the entry point repeat the call -- ride_failed / with_fuse_fallback; pace_single ends the loop on the same word)
      if (*reinterpret_cast<volatile uint64_t*>(h->hscal + 15) != 0) return 0;
      hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess) {
        if (reached()) break;
        int32_t d = 0, it = 0;
        HIPCHK(h, hipMemcpy(&d, dev_done, 4, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(&it, dev_iter, 4, hipMemcpyDeviceToHost));
        p->done = d;
        p->iter = it;
        break;
      } else if (q != hipErrorNotReady) {
        h->err = std::string("stream failed while iterating: ") + hipGetErrorString(q);
        return FPSQ_ERR_HIP;
      }
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > 120.0) {
        h->err = "timeout waiting for device progress";
        return FPSQ_ERR_TIMEOUT;
      }
      if (el > 0.002) std::this_thread::yield();
    }
  }
  return 0;
}

}  // namespace
