// fpsq_dense.hip -- host side of the dense-block direct back-end (C ABI: include/fpsq.h, "dense" section).
#include "../../include/fpsq.h"
#include "fpsq_dense.hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace fpsq;

// What the dense and the banded direct handle share: everything around their numeric cores (storage and formation of M, the
// elimination order).  Each handle derives from it and adds only its own storage.
struct DirectCore {
  const char* name = "";  // "dense" / "band": prefix of the state errors
  int64_t n = 0, m = 0, mpad = 0, nb = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  bool factored = false;
  double* invs = nullptr;   // nb inverses of the diagonal 128 x 128 blocks of L
  double* invsT = nullptr;  // ... and their transposes (k_potrf_inv128m, k_trsv_step3)
  double *r2 = nullptr, *y2 = nullptr;  // [mpad][2] each: right-hand sides / solutions of the two M-solves
  double *in_a = nullptr, *in_b = nullptr, *o_p1 = nullptr, *o_p2 = nullptr, *o_q1 = nullptr, *o_q2 = nullptr;
  int* info_dev = nullptr;
  double piv_tol = 0.0, piv_reg = 0.0;  // dynamic regularisation (fpsq_*_set_regularization); reg <= 0: off
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  // the triangular sweeps in one launch each (k_trsv_chain): publication buffer, launch number, host-mapped error word
  unsigned long long* chain_pub = nullptr;
  unsigned long long* chain_err = nullptr;
  unsigned int chain_seq = 0;
  bool chain = true;         // FPSQ_TRSV_CHAIN=0: one launch per step (k_trsv_step3)
  bool chain_break = false;  // FPSQ_DEBUG_CHAIN_BREAK=1 (tests): the workgroups publish a wrong launch number
  // jac_coord! hand-over: the caller's COO entries sorted into slots (entries of A / of the CSR), duplicates grouped
  int64_t coo_nnz = -1;
  int32_t *coo_perm = nullptr, *coo_slotptr = nullptr;
  double* coo_in = nullptr;
  // device-resident evaluations (fpsq_band_qp_*): the caller's producer stream (include/fpsq.h "INPUT READINESS") and the
  // scalars of a call, device side and pinned host side
  bool in_stream_on = false;
  hipStream_t in_stream = nullptr;
  hipEvent_t ev_in = nullptr;
  double *scal = nullptr, *scal_host = nullptr;
  // the sweeps over a tile of 16 right-hand-side columns (k_trsm_chain16), allocated by the first block call: right-hand
  // sides / solutions [mpad][16], publication buffer [nb][4096] + abort word + ticket word, launch number
  double *r16 = nullptr, *y16 = nullptr;
  unsigned long long* blk_pub = nullptr;
  unsigned int blk_seq = 0;
  std::vector<void*> allocs;
};

namespace {
// COO triplets (any order, duplicates allowed, `base`-based) -> row-major sorted slots.  order[k]: the caller's index of the
// k-th sorted entry (stable: duplicates keep the caller's order); slotptr: one range of sorted entries per distinct (row,
// col); srow / scol: the slots' coordinates.  Returns an error text, empty on success.
std::string coo_sort(int64_t m, int64_t n, int64_t nnz, const int64_t* rows, const int64_t* cols, int32_t base,
                     std::vector<int32_t>& order, std::vector<int32_t>& slotptr, std::vector<int32_t>& srow,
                     std::vector<int32_t>& scol) {
  std::vector<int32_t> cnt(m + 1, 0);
  for (int64_t k = 0; k < nnz; ++k) {
    const int64_t r = rows[k] - base, c = cols[k] - base;
    if (r < 0 || r >= m || c < 0 || c >= n) return "COO index out of range";
    cnt[r + 1]++;
  }
  for (int64_t i = 0; i < m; ++i) cnt[i + 1] += cnt[i];
  order.resize(nnz);
  {
    std::vector<int32_t> next(cnt.begin(), cnt.end() - 1);
    for (int64_t k = 0; k < nnz; ++k) order[next[rows[k] - base]++] = (int32_t)k;
  }
  for (int64_t i = 0; i < m; ++i)
    std::stable_sort(order.begin() + cnt[i], order.begin() + cnt[i + 1],
                     [&](int32_t a, int32_t b) { return cols[a] < cols[b]; });
  slotptr.assign(1, 0);
  srow.clear();
  scol.clear();
  for (int64_t i = 0; i < m; ++i)
    for (int32_t k = cnt[i]; k < cnt[i + 1]; ++k) {
      const int64_t c = cols[order[k]] - base;
      if (k > cnt[i] && c == cols[order[k - 1]] - base) {
        slotptr.back() = k + 1;
      } else {
        srow.push_back((int32_t)i);
        scol.push_back((int32_t)c);
        slotptr.push_back(k + 1);
      }
    }
  return "";
}

#define CHK(c, call)                                                           \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) {                                                    \
      (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);            \
      return FPSQ_ERR_HIP;                                                     \
    }                                                                          \
  } while (0)

template <class T>
int dalloc(DirectCore* c, T** p, size_t count) {
  void* q = nullptr;
  CHK(c, hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
  c->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

// Set-up of the shared part on the handle's device (n, m, mpad, nb and the stream are the create function's: it owns the
// error texts): events, the buffers every solve uses (`nlen`: the stored length of an n-vector), the chain publication
// buffer, the host-mapped error word, the two environment switches.  Non-zero: failed, c->err says why.
int core_setup(DirectCore* c, int64_t nlen) {
  hipEventCreate(&c->e0);
  hipEventCreate(&c->e1);
  hipEventCreate(&c->e2);
  const size_t inv_len = (size_t)c->nb * kDB * kDB;
  int rc = dalloc(c, &c->invs, inv_len) | dalloc(c, &c->invsT, inv_len);
  if (!rc) {  // k_potrf_inv128m writes the non-zero triangles only
    hipMemset(c->invs, 0, inv_len * 8);
    hipMemset(c->invsT, 0, inv_len * 8);
  }
  rc |= dalloc(c, &c->r2, (size_t)c->mpad * 2) | dalloc(c, &c->y2, (size_t)c->mpad * 2);
  rc |= dalloc(c, &c->in_a, (size_t)nlen) | dalloc(c, &c->in_b, (size_t)std::max(nlen, c->mpad));
  rc |= dalloc(c, &c->o_p1, (size_t)nlen) | dalloc(c, &c->o_p2, (size_t)nlen);
  rc |= dalloc(c, &c->o_q1, (size_t)c->mpad) | dalloc(c, &c->o_q2, (size_t)c->mpad) | dalloc(c, &c->info_dev, 4);
  const size_t pub_len = (size_t)c->nb * 512 + 8;  // (+ the abort word)
  rc |= dalloc(c, &c->chain_pub, pub_len);
  if (!rc) hipMemset(c->chain_pub, 0, pub_len * 8);
  if (hipHostMalloc((void**)&c->chain_err, 8, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) rc = 1;
  else *c->chain_err = 0;
  if (const char* e = getenv("FPSQ_TRSV_CHAIN")) c->chain = atoi(e) != 0;
  if (const char* e = getenv("FPSQ_DEBUG_CHAIN_BREAK")) c->chain_break = atoi(e) != 0;
  return rc;
}

// ... and its tear-down, the stream included; the handle itself is the caller's to delete
void core_teardown(DirectCore* c) {
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  for (void* p : c->allocs) hipFree(p);
  if (c->chain_err) hipHostFree(c->chain_err);
  if (c->scal_host) hipHostFree(c->scal_host);
  if (c->ev_in) hipEventDestroy(c->ev_in);
  if (c->e0) hipEventDestroy(c->e0);
  if (c->e1) hipEventDestroy(c->e1);
  if (c->e2) hipEventDestroy(c->e2);
  if (c->stream) hipStreamDestroy(c->stream);
}

int set_regularization(DirectCore* c, double tol, double reg) {
  if (!c || !(tol >= 0.0)) return FPSQ_ERR_ARG;
  c->piv_tol = tol;
  c->piv_reg = reg;
  return FPSQ_OK;
}

// jac_coord! hand-over: the caller's values (host or device) into `nslots` sorted slots of `out` (at target[slot] when given),
// duplicates summed in the caller's order; left in flight on c->stream
int coo_to_slots(DirectCore* c, const double* vals, const int64_t* target, double* out, int64_t nslots) {
  CHK(c, hipMemcpyAsync(c->coo_in, vals, (size_t)c->coo_nnz * 8, hipMemcpyDefault, c->stream));
  hipLaunchKernelGGL(k_coo_to_slots, dim3((unsigned)std::min<int64_t>((nslots + 255) / 256, 4096)), dim3(256), 0, c->stream,
                     c->coo_in, c->coo_perm, c->coo_slotptr, target, out, nslots);
  return FPSQ_OK;
}

// potrf + inverse of diagonal block k (at Mkk, leading dimension ld) on stream q; returns the inverse
double* launch_potrf(DirectCore* c, hipStream_t q, double* Mkk, int ld, int k) {
  double* inv = c->invs + (size_t)k * kDB * kDB;
  hipLaunchKernelGGL(k_potrf_inv128m, dim3(1), dim3(kPotrfThreads5), kPotrfLds5, q, Mkk, ld, inv,
                     c->invsT + (size_t)k * kDB * kDB, k * kDB, c->info_dev, c->piv_tol, c->piv_reg);
  return inv;
}

// End of a factorisation whose caller recorded e0 (start) and e1 (M formed) on c->stream: device times, regularised pivots,
// `factored`.  *pivot: first non-positive pivot row (1-based, stored numbering; 0: none).  Returns 1 (soft) when there is
// one: M not positive definite (the reference warns and goes on, src/solve_linear_system.jl:242-246).
int factor_end(DirectCore* c, double* form_ms, double* chol_ms, int64_t* regularized, int32_t* pivot) {
  hipEventRecord(c->e2, c->stream);
  int32_t hinfo[2] = {0, 0};
  CHK(c, hipMemcpyAsync(hinfo, c->info_dev, 8, hipMemcpyDeviceToHost, c->stream));
  CHK(c, hipStreamSynchronize(c->stream));
  float a = 0.f, b = 0.f;
  hipEventElapsedTime(&a, c->e0, c->e1);
  hipEventElapsedTime(&b, c->e1, c->e2);
  *form_ms = a;
  *chol_ms = b;
  *regularized = hinfo[1];
  *pivot = hinfo[0];
  c->factored = hinfo[0] == 0;
  return hinfo[0] == 0 ? FPSQ_OK : 1;
}

// The two triangular sweeps in one launch each: c->r2 <- M^-1 c->r2 via L y = r (into c->y2), L' q = y, with the factor at
// M (leading dimension ld).  band_w / chain_safe / chain_bw: the band geometry, 0 / 0 / 0 for a full lower triangle.
// (tickets: word 1 behind the publication buffer counts every workgroup of every sweep of this handle, nb per launch)
void chain_sweeps(DirectCore* c, const double* M, int ld, int band_w, int chain_safe, int chain_bw) {
  const int nb = (int)c->nb;
  ChainArgs a{c->chain_pub, 0, 0, nb, band_w, chain_safe, chain_bw, c->chain_err, c->chain_pub + (size_t)nb * 512 + 1, 0};
  auto next = [&] {
    a.seq = ++c->chain_seq;
    a.pubseq = c->chain_break ? ~a.seq : a.seq;
    a.ticket_base = (unsigned long long)(c->chain_seq - 1) * nb;
  };
  next();
  hipLaunchKernelGGL(k_trsv_chain<true>, dim3(nb), dim3(256), 0, c->stream, M, ld, c->invs, c->invsT, c->r2, c->y2, a);
  next();
  hipLaunchKernelGGL(k_trsv_chain<false>, dim3(nb), dim3(256), 0, c->stream, M, ld, c->invs, c->invsT, c->y2, c->r2, a);
}

// The same for a tile of 16 columns on the banded factor: c->r16 <- M^-1 c->r16 (via c->y16), one launch per sweep.  The
// tickets of these launches are counted in the word behind this publication buffer's abort word, blk_seq numbers them.
// chain16_setup allocates the buffers at the first call (they are freed with the handle); non-zero: failed.
int chain16_setup(DirectCore* c) {
  if (c->blk_pub) return FPSQ_OK;
  const size_t pub_len = (size_t)c->nb * kBlkPub + 8;
  unsigned long long* pub = nullptr;
  if (dalloc(c, &c->r16, (size_t)c->mpad * kBlkCols) || dalloc(c, &c->y16, (size_t)c->mpad * kBlkCols) ||
      dalloc(c, &pub, pub_len))
    return FPSQ_ERR_HIP;
  CHK(c, hipMemsetAsync(pub, 0, pub_len * 8, c->stream));
  c->blk_pub = pub;
  return FPSQ_OK;
}

void chain_sweeps16(DirectCore* c, const double* Mb, int band_w, int chain_safe, int chain_bw) {
  const int nb = (int)c->nb;
  ChainArgs a{c->blk_pub, 0, 0, nb, band_w, chain_safe, chain_bw, c->chain_err, c->blk_pub + (size_t)nb * kBlkPub + 1, 0};
  auto next = [&] {
    a.seq = ++c->blk_seq;
    a.pubseq = c->chain_break ? ~a.seq : a.seq;
    a.ticket_base = (unsigned long long)(c->blk_seq - 1) * nb;
  };
  next();
  hipLaunchKernelGGL(k_trsm_chain16<true>, dim3(nb), dim3(256), 0, c->stream, Mb, c->invs, c->invsT, c->r16, c->y16, a);
  next();
  hipLaunchKernelGGL(k_trsm_chain16<false>, dim3(nb), dim3(256), 0, c->stream, Mb, c->invs, c->invsT, c->y16, c->r16, a);
}

// Start of a solve_two_* call: argument and state checks, the two right-hand sides staged in in_a / in_b (rhs1: n doubles,
// rhs2: m when `mixed`, else n), e0
int solve_begin(DirectCore* c, bool mixed, const double* rhs1, const double* rhs2, const double* p1, const double* q1,
                const double* p2, const double* q2) {
  if (!c || !rhs1 || !rhs2 || !p1 || !q1 || !p2 || !q2) return FPSQ_ERR_ARG;
  if (!c->factored) {
    c->err = std::string(c->name) + "_solve: no valid factorisation";
    return FPSQ_ERR_STATE;
  }
  hipSetDevice(c->device);
  CHK(c, hipMemcpyAsync(c->in_a, rhs1, (size_t)c->n * 8, hipMemcpyDefault, c->stream));
  CHK(c, hipMemcpyAsync(c->in_b, rhs2, (size_t)(mixed ? c->m : c->n) * 8, hipMemcpyDefault, c->stream));
  hipEventRecord(c->e0, c->stream);
  return FPSQ_OK;
}

// ... and its end, the results being in flight in o_p1 .. o_q2: e1, the copies to the caller, the check of the sweeps' error word
int solve_end(DirectCore* c, double* p1, double* q1, double* p2, double* q2, double* solve_ms) {
  hipStream_t s = c->stream;
  hipEventRecord(c->e1, s);
  CHK(c, hipMemcpyAsync(p1, c->o_p1, (size_t)c->n * 8, hipMemcpyDefault, s));
  CHK(c, hipMemcpyAsync(p2, c->o_p2, (size_t)c->n * 8, hipMemcpyDefault, s));
  CHK(c, hipMemcpyAsync(q1, c->o_q1, (size_t)c->m * 8, hipMemcpyDefault, s));
  CHK(c, hipMemcpyAsync(q2, c->o_q2, (size_t)c->m * 8, hipMemcpyDefault, s));
  CHK(c, hipStreamSynchronize(s));
  if (c->chain_err && *c->chain_err) {
    *c->chain_err = 0;
    c->err = "triangular sweep: a block's solution did not arrive (bounded wait expired); FPSQ_TRSV_CHAIN=0 avoids the path";
    return FPSQ_ERR_TIMEOUT;
  }
  float ms = 0.f;
  hipEventElapsedTime(&ms, c->e0, c->e1);
  *solve_ms = ms;
  return FPSQ_OK;
}

// ---- around the kernels of a device-resident evaluation (fpsq_band_qp_*); nothing here knows how M is stored

int set_input_stream(DirectCore* c, int32_t enabled, void* hip_stream) {
  if (!c) return FPSQ_ERR_ARG;
  hipSetDevice(c->device);
  if (enabled && !c->ev_in) CHK(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
  c->in_stream_on = enabled != 0;
  c->in_stream = (hipStream_t)hip_stream;
  return FPSQ_OK;
}

// the handle's stream waits (event, no host block) for everything enqueued so far on the registered stream
int wait_input(DirectCore* c) {
  if (!c->in_stream_on) return FPSQ_OK;
  CHK(c, hipEventRecord(c->ev_in, c->in_stream));
  CHK(c, hipStreamWaitEvent(c->stream, c->ev_in, 0));
  return FPSQ_OK;
}

// true when p is device memory of the handle's GPU (kernels then use it in place)
bool on_device(const DirectCore* c, const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // plain host memory: not an error
    return false;
  }
  return a.type == hipMemoryTypeDevice && a.device == c->device;
}

// An input vector as the kernels read it: in place when it lives on the handle's GPU, else copied into `stage`
int arg_in(DirectCore* c, const double* p, double* stage, size_t len, const double** out) {
  *out = p;
  if (!p || on_device(c, p)) return FPSQ_OK;
  CHK(c, hipMemcpyAsync(stage, p, len * 8, hipMemcpyDefault, c->stream));
  *out = stage;
  return FPSQ_OK;
}

// ... where they write an output vector (null stays null), and the copy back of one that was staged
double* arg_out(DirectCore* c, double* p, double* stage) { return !p || on_device(c, p) ? p : stage; }

int arg_back(DirectCore* c, double* p, const double* wrote, size_t len) {
  if (!p || wrote == p) return FPSQ_OK;
  CHK(c, hipMemcpyAsync(p, wrote, len * 8, hipMemcpyDefault, c->stream));
  return FPSQ_OK;
}

// Start of an evaluation on the cached factor: state check, input ordering, e0
int eval_begin(DirectCore* c) {
  if (!c->factored) {
    c->err = std::string(c->name) + "_solve: no valid factorisation";
    return FPSQ_ERR_STATE;
  }
  hipSetDevice(c->device);
  if (int rc = wait_input(c)) return rc;
  hipEventRecord(c->e0, c->stream);
  return FPSQ_OK;
}

// ... and its end: e1, the one device-to-host transfer of the call's `nscal` scalars (c->scal -> c->scal_host), the
// synchronisation that makes the outputs complete, the check of the sweeps' error word
int eval_end(DirectCore* c, int nscal, double* solve_ms) {
  hipStream_t s = c->stream;
  hipEventRecord(c->e1, s);
  if (nscal > 0) CHK(c, hipMemcpyAsync(c->scal_host, c->scal, (size_t)nscal * 8, hipMemcpyDeviceToHost, s));
  CHK(c, hipStreamSynchronize(s));
  if (c->chain_err && *c->chain_err) {
    *c->chain_err = 0;
    c->err = "triangular sweep: a block's solution did not arrive (bounded wait expired); FPSQ_TRSV_CHAIN=0 avoids the path";
    return FPSQ_ERR_TIMEOUT;
  }
  float ms = 0.f;
  hipEventElapsedTime(&ms, c->e0, c->e1);
  *solve_ms = ms;
  return FPSQ_OK;
}

// lanes that share a row in the product kernels of the evaluations: the largest power of two <= the mean row length, 1 .. 64
int lane_group(int64_t nnz, int64_t rows) {
  const int64_t mean = rows > 0 ? nnz / rows : 1;
  int lg = 1;
  while (lg < 64 && 2 * lg <= mean) lg *= 2;
  return lg;
}

// runs the statement(s) with the compile-time constant LG = lg (a value lane_group returns)
#define WITH_LANE_GROUP(lg, ...)                            \
  switch (lg) {                                             \
    case 1: { constexpr int LG = 1; __VA_ARGS__; } break;    \
    case 2: { constexpr int LG = 2; __VA_ARGS__; } break;    \
    case 4: { constexpr int LG = 4; __VA_ARGS__; } break;    \
    case 8: { constexpr int LG = 8; __VA_ARGS__; } break;    \
    case 16: { constexpr int LG = 16; __VA_ARGS__; } break;  \
    case 32: { constexpr int LG = 32; __VA_ARGS__; } break;  \
    default: { constexpr int LG = 64; __VA_ARGS__; } break;  \
  }
}  // namespace

// ===================================================================================================== dense M

struct fpsq_dense_s : DirectCore {
  int64_t npad = 0;
  bool have_jac = false;
  double* A = nullptr;  // mpad x npad, row-major, zero padded
  double* M = nullptr;  // mpad x mpad: lower triangle holds the Cholesky factor after factorize
  double *x2 = nullptr, *part = nullptr;  // [npad][2], gemvt partials
  int nchunk = 16;
  // (one generation of every kernel is left in the source: the sixteen-wave Gram product k_gemm_nt_f64_w16, the diagonal-block
  // kernel k_potrf_inv128m, the single-round-trip step products k_gemm128_lds and the latency-organised solve step
  // k_trsv_step3.  Their predecessors, the look-ahead and split-K variants -- all measured slower, DESIGN.md section 7 --
  // and the environment switches that selected them were removed in round 3.)
  // fpsq_dense_set_structure_coo: where each sorted slot lies in A
  int64_t coo_slots = 0;
  int64_t* coo_target = nullptr;
  fpsq_dense_info info{};
};

namespace {
thread_local std::string g_dense_create_error;

// q (m x 2 in d->r2, overwritten) <- M^-1 r2 via L y = r, L' q = y; the solution ends up in d->r2
void dense_sweeps(fpsq_dense d) {
  if (d->chain) return chain_sweeps(d, d->M, (int)d->mpad, 0, 0, 0);
  hipStream_t s = d->stream;
  const int nb = (int)d->nb, ld = (int)d->mpad;
  for (int k = 0; k < nb; ++k)
    hipLaunchKernelGGL(k_trsv_step3<true>, dim3(nb - k), dim3(256), 0, s, d->M, ld, d->invs, d->invsT, d->r2, d->y2, k, 0);
  for (int k = nb - 1; k >= 0; --k)
    hipLaunchKernelGGL(k_trsv_step3<false>, dim3(k + 1), dim3(256), 0, s, d->M, ld, d->invs, d->invsT, d->y2, d->r2, k, 0);
}

// common tail: Q in d->r2 ([mpad][2]); P = [a0, a1] - A' Q
int dense_finish(fpsq_dense d, const double* a0, const double* a1, double* p1, double* q1, double* p2, double* q2) {
  hipStream_t s = d->stream;
  const int rows_per_chunk = (int)((d->mpad + d->nchunk - 1) / d->nchunk);
  hipLaunchKernelGGL(k_dense_gemvt_part<2>, dim3((unsigned)((d->npad + 255) / 256), d->nchunk), dim3(256), 0, s, d->A,
                     (int)d->npad, (int)d->mpad, (int)d->npad, d->r2, d->part, rows_per_chunk);
  hipLaunchKernelGGL(k_dense_finish_p, dim3((unsigned)((d->n + 255) / 256)), dim3(256), 0, s, d->part, d->nchunk,
                     (int)d->npad, (int)d->n, a0, a1, d->o_p1, d->o_p2);
  hipLaunchKernelGGL(k_dense_unpack2, dim3((unsigned)((d->m + 255) / 256)), dim3(256), 0, s, d->r2, d->o_q1, d->o_q2,
                     (int)d->m);
  return solve_end(d, p1, q1, p2, q2, &d->info.last_solve_ms);
}
}  // namespace

extern "C" {

const char* fpsq_dense_last_error(fpsq_dense d) { return d ? d->err.c_str() : g_dense_create_error.c_str(); }

int fpsq_dense_create(fpsq_dense* out, int64_t n, int64_t m, int32_t device) {
  if (!out || n <= 0 || m <= 0 || n > (1 << 20) || m > (1 << 16)) {
    g_dense_create_error = "fpsq_dense_create: bad arguments (n <= 2^20, m <= 2^16)";
    return FPSQ_ERR_ARG;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    g_dense_create_error = std::string("fpsq_dense_create: no HIP device (") + hipGetErrorString(e) +
                           "); libfpsq has no CPU fallback";
    return FPSQ_ERR_HIP;
  }
  fpsq_dense d = new fpsq_dense_s();
  d->n = n;
  d->m = m;
  d->device = device;
  d->name = "dense";
  d->mpad = (m + kDB - 1) / kDB * kDB;
  d->npad = (n + kW16Kd - 1) / kW16Kd * kW16Kd;  // whole k-stages of the Gram product
  d->nb = d->mpad / kDB;
  d->nchunk = (int)std::min<int64_t>(32, d->nb * 4);
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) {
    g_dense_create_error = "fpsq_dense_create: cannot initialise device";
    delete d;
    return FPSQ_ERR_HIP;
  }
  int rc = core_setup(d, d->npad);
  rc |= dalloc(d, &d->A, (size_t)d->mpad * d->npad);
  rc |= dalloc(d, &d->M, (size_t)d->mpad * d->mpad);
  rc |= dalloc(d, &d->x2, (size_t)d->npad * 2);
  rc |= dalloc(d, &d->part, (size_t)d->nchunk * d->npad * 2);
  if (rc) {
    g_dense_create_error = d->err;
    fpsq_dense_destroy(d);
    return FPSQ_ERR_HIP;
  }
  // on the solver's own (non-blocking) stream: a null-stream memset is not ordered against it
  hipMemsetAsync(d->A, 0, (size_t)d->mpad * d->npad * 8, d->stream);
  hipStreamSynchronize(d->stream);
  hipFuncSetAttribute((const void*)k_potrf_inv128m, hipFuncAttributeMaxDynamicSharedMemorySize, kPotrfLds5);
  hipFuncSetAttribute((const void*)k_gemm128_lds<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kG128Lds0);
  hipFuncSetAttribute((const void*)k_gemm128_lds<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kG128Lds1);
  hipFuncSetAttribute((const void*)k_gemm_nt_f64_w16<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kW16Lds);
  d->info.n = n;
  d->info.m = m;
  *out = d;
  return FPSQ_OK;
}

int fpsq_dense_destroy(fpsq_dense d) {
  if (!d) return FPSQ_ERR_ARG;
  core_teardown(d);
  delete d;
  return FPSQ_OK;
}

int fpsq_dense_set_jacobian(fpsq_dense d, const double* a_rowmajor) {
  if (!d || !a_rowmajor) return FPSQ_ERR_ARG;
  hipSetDevice(d->device);
  CHK(d, hipMemcpy2DAsync(d->A, (size_t)d->npad * 8, a_rowmajor, (size_t)d->n * 8, (size_t)d->n * 8, (size_t)d->m,
                          hipMemcpyDefault, d->stream));
  CHK(d, hipStreamSynchronize(d->stream));
  d->have_jac = true;
  d->factored = false;
  return FPSQ_OK;
}

int fpsq_dense_set_structure_coo(fpsq_dense d, int64_t nnz, const int64_t* rows, const int64_t* cols, int32_t index_base) {
  if (!d || nnz < 0 || nnz >= INT32_MAX || (nnz > 0 && (!rows || !cols))) return FPSQ_ERR_ARG;
  hipSetDevice(d->device);
  std::vector<int64_t> r(nnz), c(nnz);
  if (nnz) {
    CHK(d, hipMemcpy(r.data(), rows, (size_t)nnz * 8, hipMemcpyDefault));
    CHK(d, hipMemcpy(c.data(), cols, (size_t)nnz * 8, hipMemcpyDefault));
  }
  std::vector<int32_t> order, slotptr, srow, scol;
  const std::string msg = coo_sort(d->m, d->n, nnz, r.data(), c.data(), index_base, order, slotptr, srow, scol);
  if (!msg.empty()) {
    d->err = "dense_set_structure_coo: " + msg;
    return FPSQ_ERR_ARG;
  }
  const int64_t ns = (int64_t)srow.size();
  std::vector<int64_t> target(std::max<int64_t>(ns, 1));
  for (int64_t i = 0; i < ns; ++i) target[i] = (int64_t)srow[i] * d->npad + scol[i];
  const bool dup = ns != nnz;
  // a second structure call replaces the first one's buffers (and must not keep its slot table when the new pattern has no
  // duplicates: k_coo_to_slots takes a non-null table for one)
  for (void** q : {(void**)&d->coo_perm, (void**)&d->coo_in, (void**)&d->coo_target, (void**)&d->coo_slotptr}) {
    if (!*q) continue;
    auto it = std::find(d->allocs.begin(), d->allocs.end(), *q);
    if (it != d->allocs.end()) d->allocs.erase(it);
    hipFree(*q);
    *q = nullptr;
  }
  d->coo_nnz = -1;
  if (dalloc(d, &d->coo_perm, (size_t)std::max<int64_t>(nnz, 1)) || dalloc(d, &d->coo_in, (size_t)std::max<int64_t>(nnz, 1)) ||
      dalloc(d, &d->coo_target, target.size()) || (dup && dalloc(d, &d->coo_slotptr, slotptr.size())))
    return FPSQ_ERR_HIP;
  if (nnz) CHK(d, hipMemcpy(d->coo_perm, order.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
  CHK(d, hipMemcpy(d->coo_target, target.data(), target.size() * 8, hipMemcpyHostToDevice));
  if (dup) CHK(d, hipMemcpy(d->coo_slotptr, slotptr.data(), slotptr.size() * 4, hipMemcpyHostToDevice));
  // entries outside the pattern are zero for good: the value hand-over only rewrites the pattern's slots
  CHK(d, hipMemsetAsync(d->A, 0, (size_t)d->mpad * d->npad * 8, d->stream));
  CHK(d, hipStreamSynchronize(d->stream));
  d->coo_nnz = nnz;
  d->coo_slots = ns;
  d->have_jac = false;
  return FPSQ_OK;
}

int fpsq_dense_set_jacobian_coo(fpsq_dense d, const double* vals) {
  if (!d || d->coo_nnz < 0 || (!vals && d->coo_nnz > 0)) {
    if (d) d->err = "dense_set_jacobian_coo: structure not set (fpsq_dense_set_structure_coo) or null values";
    return FPSQ_ERR_ARG;
  }
  hipSetDevice(d->device);
  if (d->coo_nnz > 0)
    if (int rc = coo_to_slots(d, vals, d->coo_target, d->A, d->coo_slots)) return rc;
  CHK(d, hipStreamSynchronize(d->stream));
  d->have_jac = true;
  d->factored = false;
  return FPSQ_OK;
}

int fpsq_dense_factorize(fpsq_dense d, double delta, int32_t* info) {
  if (!d || !(delta >= 0.0)) return FPSQ_ERR_ARG;
  if (!d->have_jac) {
    d->err = "dense_factorize: Jacobian not set";
    return FPSQ_ERR_STATE;
  }
  hipSetDevice(d->device);
  hipStream_t s = d->stream;
  const int nb = (int)d->nb, ld = (int)d->mpad;
  CHK(d, hipMemsetAsync(d->info_dev, 0, 8, s));
  hipEventRecord(d->e0, s);
  // M = A A' (lower tiles) on the fp64 matrix cores, then + delta I
  hipLaunchKernelGGL(k_gemm_nt_f64_w16<true>, dim3(nb, nb), dim3(1024), kW16Lds, s, d->M, ld, d->A, (int)d->npad, d->A,
                     (int)d->npad, (int)d->npad, 1.0, 0.0, 0, (size_t)0);
  hipLaunchKernelGGL(k_dense_diag, dim3((unsigned)((d->mpad + 255) / 256)), dim3(256), 0, s, d->M, ld, (int)d->m, (int)d->mpad,
                     delta);
  hipEventRecord(d->e1, s);
  // right-looking blocked Cholesky, block 128: potrf + inverse of the diagonal block (one workgroup), panel
  // L_ik = M_ik Linv_kk' and trailing update M_ij -= L_ik L_jk' on the matrix cores
  for (int k = 0; k < nb; ++k) {
    double* Mkk = d->M + (size_t)k * kDB * ld + (size_t)k * kDB;
    double* inv = launch_potrf(d, s, Mkk, ld, k);
    const int rem = nb - k - 1;
    if (rem > 0) {  // the K = 128 products of the step, each in one memory round trip (k_gemm128_lds)
      double* panel = d->M + (size_t)(k + 1) * kDB * ld + (size_t)k * kDB;
      double* trail = d->M + (size_t)(k + 1) * kDB * ld + (size_t)(k + 1) * kDB;
      hipLaunchKernelGGL(k_gemm128_lds<1>, dim3(1, 4 * rem), dim3(1024), kG128Lds1, s, panel, ld, panel, ld, inv, kDB,
                         BlockStrides{});
      hipLaunchKernelGGL(k_gemm128_lds<0>, dim3(2 * rem, 2 * rem), dim3(1024), kG128Lds0, s, trail, ld, panel, ld, panel, ld,
                         BlockStrides{});
    }
  }
  int32_t pivot = 0;
  const int rc = factor_end(d, &d->info.last_syrk_ms, &d->info.last_chol_ms, &d->info.regularized_pivots, &pivot);
  if (rc >= 0 && info) *info = pivot;
  return rc;
}

int fpsq_dense_set_regularization(fpsq_dense d, double tol, double reg) { return set_regularization(d, tol, reg); }

int fpsq_dense_solve_two_mixed(fpsq_dense d, const double* rhs1, const double* rhs2, double* p1, double* q1, double* p2,
                               double* q2) {
  if (int rc = solve_begin(d, true, rhs1, rhs2, p1, q1, p2, q2)) return rc;
  hipStream_t s = d->stream;
  // r = [A g, -c]:  q1 = M^-1 A g,  q2 = -M^-1 c   
  hipLaunchKernelGGL(k_dense_pack2, dim3((unsigned)((d->npad + 255) / 256)), dim3(256), 0, s, d->in_a, 1.0,
                     (const double*)nullptr, 0.0, d->x2, (int)d->n, (int)d->npad);
  hipLaunchKernelGGL(k_dense_gemv<2>, dim3((unsigned)((d->mpad + 3) / 4)), dim3(256), 0, s, d->A, (int)d->npad,
                     (int)d->mpad, (int)d->npad, d->x2, 1.0, (const double*)nullptr, 0.0, d->y2);
  hipLaunchKernelGGL(k_dense_unpack2, dim3((unsigned)((d->mpad + 255) / 256)), dim3(256), 0, s, d->y2, d->o_q1, d->o_q2,
                     (int)d->mpad);
  hipLaunchKernelGGL(k_dense_pack2, dim3((unsigned)((d->mpad + 255) / 256)), dim3(256), 0, s, d->o_q1, 1.0, d->in_b, -1.0,
                     d->r2, (int)d->m, (int)d->mpad);
  dense_sweeps(d);
  return dense_finish(d, d->in_a, nullptr, p1, q1, p2, q2);
}

int fpsq_dense_solve_two_least_squares(fpsq_dense d, const double* rhs1, const double* rhs2, double* p1, double* q1,
                                       double* p2, double* q2) {
  if (int rc = solve_begin(d, false, rhs1, rhs2, p1, q1, p2, q2)) return rc;
  hipStream_t s = d->stream;
  hipLaunchKernelGGL(k_dense_pack2, dim3((unsigned)((d->npad + 255) / 256)), dim3(256), 0, s, d->in_a, 1.0, d->in_b, 1.0,
                     d->x2, (int)d->n, (int)d->npad);
  hipLaunchKernelGGL(k_dense_gemv<2>, dim3((unsigned)((d->mpad + 3) / 4)), dim3(256), 0, s, d->A, (int)d->npad,
                     (int)d->mpad, (int)d->npad, d->x2, 1.0, (const double*)nullptr, 0.0, d->r2);
  dense_sweeps(d);
  return dense_finish(d, d->in_a, d->in_b, p1, q1, p2, q2);
}

int fpsq_dense_get_factor(fpsq_dense d, double* l_out) {
  if (!d || !l_out) return FPSQ_ERR_ARG;
  hipSetDevice(d->device);
  CHK(d, hipMemcpy2D(l_out, (size_t)d->m * 8, d->M, (size_t)d->mpad * 8, (size_t)d->m * 8, (size_t)d->m, hipMemcpyDefault));
  return FPSQ_OK;
}

int fpsq_dense_get_info(fpsq_dense d, fpsq_dense_info* info) {
  if (!d || !info) return FPSQ_ERR_ARG;
  *info = d->info;
  return FPSQ_OK;
}
}  // extern "C"

// ===================================================================================== sparse direct path (block band)

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
  // Ptv [n][8] (sparse Q only), and the staging of host-resident blocks (rhs1 / V, rhs2, p1 / HV, p2: 8 n; q1, q2: 8 m)
  double *blk_xg = nullptr, *blk_keep = nullptr, *blk_tv = nullptr;
  double* blk_stage[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool have_vals = false;    // a factorisation has put the Jacobian's values into vals / t_vals (fpsq_band_jac_mul, fpsq_band_qp_*)
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
std::string band_order(int64_t n, int64_t m, std::vector<int32_t>& rp, std::vector<int32_t>& ci, std::vector<int32_t>& rperm_h,
                       std::vector<int32_t>& vperm_h, int& chain_safe, int& chain_bw) {
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

inline size_t blk_off(const fpsq_band b, int64_t i, int64_t j) {  // block (i, j), i - (band_w - 1) <= j <= i
  return ((size_t)i * b->band_w + (size_t)(j - i + b->band_w - 1)) * kDB * kDB;
}

// q (in b->r2, [mpad][2]) <- M^-1 r2 with the banded factor; result in b->r2
void band_solve(fpsq_band b) {
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
  hipLaunchKernelGGL(k_csr_mv2, dim3((unsigned)((b->n + 255) / 256)), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals,
                     b->r2, b->atq, (int)b->n);
  hipLaunchKernelGGL(k_band_finish, dim3((unsigned)((b->n + 255) / 256)), dim3(256), 0, s, b->atq, b->in_a, a1, b->o_p1,
                     b->o_p2, (int)b->n);
  if (b->reordered)  // back to the caller's row order
    hipLaunchKernelGGL(k_unpack2_scatter, dim3((unsigned)((b->m + 255) / 256)), dim3(256), 0, s, b->r2, b->rperm, b->o_q1,
                       b->o_q2, (int)b->m);
  else
    hipLaunchKernelGGL(k_dense_unpack2, dim3((unsigned)((b->m + 255) / 256)), dim3(256), 0, s, b->r2, b->o_q1, b->o_q2,
                       (int)b->m);
  return solve_end(b, p1, q1, p2, q2, &b->info.last_solve_ms);
}
}  // namespace

extern "C" {

const char* fpsq_band_last_error(fpsq_band b) { return b ? b->err.c_str() : g_band_create_error.c_str(); }

int fpsq_band_analyze(int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t* row_perm,
                      fpsq_band_info* info) {
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
  int chain_safe = 0, chain_bw = 0;
  const std::string msg = band_order(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw);
  if (!msg.empty()) {
    g_band_create_error = msg;
    return FPSQ_ERR_ARG;
  }
  if (row_perm)
    for (int64_t p = 0; p < m; ++p) row_perm[p] = rperm_h.empty() ? (int32_t)p : rperm_h[p];
  if (info) {
    std::vector<int32_t> lo(n, INT32_MAX), hi(n, -1);
    for (int64_t i = 0; i < m; ++i)
      for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        lo[ci[k]] = std::min(lo[ci[k]], (int32_t)(i / kDB));
        hi[ci[k]] = std::max(hi[ci[k]], (int32_t)(i / kDB));
      }
    int64_t bwb = 0;
    for (int64_t c = 0; c < n; ++c)
      if (hi[c] >= 0) bwb = std::max<int64_t>(bwb, hi[c] - lo[c]);
    const int64_t nb = (m + kDB - 1) / kDB;
    bwb = std::min(bwb, nb - 1);
    *info = fpsq_band_info{};
    info->n = n;
    info->m = m;
    info->nnz = nnz;
    info->nblocks = nb;
    info->bandwidth_blocks = bwb;
    info->factor_bytes = nb * (bwb + 1) * (int64_t)kDB * kDB * 8;
    info->reordered = rperm_h.empty() ? 0 : 1;
    info->chains = chain_safe > 0 ? 2 : 1;
  }
  return FPSQ_OK;
}

int fpsq_band_destroy(fpsq_band b) {
  if (!b) return FPSQ_ERR_ARG;
  core_teardown(b);
  if (b->evA) hipEventDestroy(b->evA);
  if (b->evB) hipEventDestroy(b->evB);
  if (b->stream2) {
    hipStreamSynchronize(b->stream2);
    hipStreamDestroy(b->stream2);
  }
  delete b;
  return FPSQ_OK;
}

int fpsq_band_create(fpsq_band* out, int64_t n, int64_t m, const int32_t* rowptr, const int32_t* colind, int32_t device) {
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
  // ---- symbolic analysis on the host (the role of ldl_analyze, src/solve_two_systems_struct.jl:344): the structure of
  // A A' + delta I is a band whose half width is the largest row distance of two entries of one column of A
  std::vector<int32_t> rp(m + 1);
  if (hipMemcpy(rp.data(), rowptr, (size_t)(m + 1) * 4, hipMemcpyDefault) != hipSuccess || rp[0] != 0) {
    g_band_create_error = "fpsq_band_create: cannot read rowptr (0-based CSR expected)";
    return FPSQ_ERR_ARG;
  }
  const int64_t nnz = rp[m];
  std::vector<int32_t> ci(std::max<int64_t>(nnz, 1));
  if (nnz > 0 && (!colind || hipMemcpy(ci.data(), colind, (size_t)nnz * 4, hipMemcpyDefault) != hipSuccess)) {
    g_band_create_error = "fpsq_band_create: cannot read colind";
    return FPSQ_ERR_ARG;
  }
  std::vector<int32_t> rperm_h, vperm_h;  // stored row / entry -> the caller's (empty: identity)
  int chain_safe = 0, chain_bw = 0;
  {
    const std::string msg = band_order(n, m, rp, ci, rperm_h, vperm_h, chain_safe, chain_bw);
    if (!msg.empty()) {
      g_band_create_error = msg;
      return FPSQ_ERR_ARG;
    }
  }
  std::vector<int32_t> cfirst(n, INT32_MAX), clast(n, -1), tcnt(n + 1, 0);
  std::vector<int2> span(m);
  std::vector<int32_t> seen(n, -1);
  bool has_dup = false;
  int maxspan = 1;
  for (int64_t i = 0; i < m; ++i) {
    if (rp[i + 1] < rp[i]) {
      g_band_create_error = "fpsq_band_create: rowptr not monotone";
      return FPSQ_ERR_ARG;
    }
    int lo = INT32_MAX, hi = -1;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
      const int32_t c = ci[k];
      if (c < 0 || c >= n) {
        g_band_create_error = "fpsq_band_create: column index out of range";
        return FPSQ_ERR_ARG;
      }
      lo = std::min(lo, c);
      hi = std::max(hi, c);
      has_dup |= seen[c] == (int32_t)i;
      seen[c] = (int32_t)i;
      cfirst[c] = std::min<int32_t>(cfirst[c], (int32_t)i);
      clast[c] = std::max<int32_t>(clast[c], (int32_t)i);
      tcnt[c + 1]++;
    }
    if (hi < 0) lo = hi = 0;
    span[i] = int2{lo, hi};
    maxspan = std::max(maxspan, hi - lo + 1);
  }
  int64_t bwb = 0;
  for (int64_t c = 0; c < n; ++c)
    if (clast[c] >= 0) bwb = std::max<int64_t>(bwb, clast[c] / kDB - cfirst[c] / kDB);
  fpsq_band b = new fpsq_band_s();
  b->name = "band";
  b->n = n;
  b->m = m;
  b->nnz = nnz;
  b->device = device;
  b->mpad = (m + kDB - 1) / kDB * kDB;
  b->nb = b->mpad / kDB;
  b->band_w = (int)std::min<int64_t>(bwb, b->nb - 1) + 1;
  b->span = maxspan;
  b->chain_safe = chain_safe;
  b->chain_bw = std::min(chain_bw, (b->band_w - 1) / 2);
  if (has_dup) {
    g_band_create_error = "fpsq_band_create: the CSR pattern has duplicate entries (sum them first)";
    delete b;
    return FPSQ_ERR_ARG;
  }
  // M is formed by columns of A (k_band_form_t) when its accumulator rows fit in LDS; otherwise by row pairs
  // (k_band_form), which needs the widest row span in LDS twice
  b->form_R = 16;
  while (b->form_R > 1 && b->form_R * b->band_w > 144) b->form_R /= 2;
  b->form_gen = b->band_w > 144 ? 1 : 2;
  if (const char* ev = std::getenv("FPSQ_BAND_FORM")) {
    const int want = std::atoi(ev);
    if (want == 1 || (want == 2 && b->band_w <= 144)) b->form_gen = want;
  }
  const size_t fbytes = (size_t)b->nb * b->band_w * kDB * kDB * 8;
  size_t free_b = 0, total_b = 0;
  hipMemGetInfo(&free_b, &total_b);
  if ((b->form_gen == 1 && (size_t)maxspan * 16 > 150 * 1024) || fbytes + 3 * ((size_t)b->nb * kDB * kDB * 8) > free_b / 10 * 9) {
    char msg[256];
    snprintf(msg, sizeof msg, "fpsq_band_create: the banded direct path does not fit this Jacobian (half bandwidth %d "
             "blocks > 143 and a row span of %d columns > 9600, or factor storage %.1f GB of %.1f GB "
             "free): use the iterative back-end", b->band_w - 1, maxspan, fbytes / 1e9, free_b / 1e9);
    g_band_create_error = msg;
    delete b;
    return FPSQ_ERR_STATE;
  }
  // transposed structure (for P = rhs - A' Q) with the value permutation
  for (int64_t c = 0; c < n; ++c) tcnt[c + 1] += tcnt[c];
  std::vector<int32_t> trow(std::max<int64_t>(nnz, 1)), tperm(std::max<int64_t>(nnz, 1)), nxt(tcnt.begin(), tcnt.end() - 1);
  for (int64_t i = 0; i < m; ++i)
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
      const int32_t t = nxt[ci[k]]++;
      trow[t] = (int32_t)i;
      tperm[t] = k;
    }
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
    g_band_create_error = "fpsq_band_create: cannot create a stream";
    delete b;
    return FPSQ_ERR_HIP;
  }
  hipStreamCreateWithFlags(&b->stream2, hipStreamNonBlocking);
  hipEventCreateWithFlags(&b->evA, hipEventDisableTiming);
  hipEventCreateWithFlags(&b->evB, hipEventDisableTiming);
  int rc = core_setup(b, n);
  const size_t nz = (size_t)std::max<int64_t>(nnz, 1);
  rc |= dalloc(b, &b->rowptr, (size_t)m + 1) | dalloc(b, &b->colind, nz) | dalloc(b, &b->vals, nz);
  rc |= dalloc(b, &b->t_rowptr, (size_t)n + 1) | dalloc(b, &b->t_colind, nz) | dalloc(b, &b->t_vals, nz);
  rc |= dalloc(b, &b->t_perm, nz) | dalloc(b, &b->rowspan, (size_t)m);
  rc |= dalloc(b, &b->Mb, (size_t)b->nb * b->band_w * kDB * kDB);
  rc |= dalloc(b, &b->xn, (size_t)n * 2) | dalloc(b, &b->atq, (size_t)n * 2) | dalloc(b, &b->ym, (size_t)b->mpad * 2);
  b->reordered = !rperm_h.empty();
  b->rperm_host = rperm_h;
  if (b->reordered)
    rc |= dalloc(b, &b->rperm, (size_t)m) | dalloc(b, &b->vperm, nz) | dalloc(b, &b->vals_in, nz) |
          dalloc(b, &b->in_bp, (size_t)b->mpad);
  if (rc) {
    g_band_create_error = b->err;
    fpsq_band_destroy(b);
    return FPSQ_ERR_HIP;
  }
  if (b->reordered) {
    hipMemcpy(b->rperm, rperm_h.data(), (size_t)m * 4, hipMemcpyHostToDevice);
    if (nnz > 0) hipMemcpy(b->vperm, vperm_h.data(), (size_t)nnz * 4, hipMemcpyHostToDevice);
  }
  hipMemcpy(b->rowptr, rp.data(), (size_t)(m + 1) * 4, hipMemcpyHostToDevice);
  hipMemcpy(b->t_rowptr, tcnt.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice);
  hipMemcpy(b->rowspan, span.data(), (size_t)m * sizeof(int2), hipMemcpyHostToDevice);
  if (nnz > 0) {
    hipMemcpy(b->colind, ci.data(), (size_t)nnz * 4, hipMemcpyHostToDevice);
    hipMemcpy(b->t_colind, trow.data(), (size_t)nnz * 4, hipMemcpyHostToDevice);
    hipMemcpy(b->t_perm, tperm.data(), (size_t)nnz * 4, hipMemcpyHostToDevice);
  }
  hipDeviceSynchronize();
  hipFuncSetAttribute((const void*)k_potrf_inv128m, hipFuncAttributeMaxDynamicSharedMemorySize, kPotrfLds5);
  hipFuncSetAttribute((const void*)k_gemm128_lds<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kG128Lds0);
  hipFuncSetAttribute((const void*)k_gemm128_lds<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kG128Lds1);
  if (b->form_gen == 1)
    hipFuncSetAttribute((const void*)k_band_form, hipFuncAttributeMaxDynamicSharedMemorySize, maxspan * 16);
  else
    hipFuncSetAttribute((const void*)k_band_form_t, hipFuncAttributeMaxDynamicSharedMemorySize,
                        b->form_R * b->band_w * kDB * 8);
  b->info.n = n;
  b->info.m = m;
  b->info.nnz = nnz;
  b->info.nblocks = b->nb;
  b->info.bandwidth_blocks = b->band_w - 1;
  b->info.reordered = b->reordered ? 1 : 0;
  b->info.chains = b->chain_safe > 0 ? 2 : 1;
  b->info.factor_bytes = (int64_t)fbytes;
  *out = b;
  return FPSQ_OK;
}

int fpsq_band_create_coo(fpsq_band* out, int64_t n, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                         int32_t index_base, int32_t device) {
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
  if (int rc = fpsq_band_create(out, n, m, rp.data(), scol.data(), device)) return rc;
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
  const int nb = (int)b->nb, W = b->band_w, bw = W - 1;
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
    hipLaunchKernelGGL(k_gather_d, dim3((unsigned)std::min<int64_t>((b->nnz + 255) / 256, 4096)), dim3(256), 0, s, b->vals,
                       b->t_perm, b->t_vals, b->nnz);
  }
  CHK(b, hipMemsetAsync(b->info_dev, 0, 8, s));
  CHK(b, hipMemsetAsync(b->Mb, 0, (size_t)nb * W * kDB * kDB * 8, s));
  hipEventRecord(b->e0, s);
  // numeric phase 1: M = A A' + delta I into the band (jac_coord! + sparse(...) of src/solve_linear_system.jl:223-233)
  if (b->form_gen == 1)
    hipLaunchKernelGGL(k_band_form, dim3(nb), dim3(256), (size_t)b->span * 16, s, b->rowptr, b->colind, b->vals, b->rowspan,
                       (int)b->m, (int)b->mpad, W, delta, b->Mb, b->span);
  else
    hipLaunchKernelGGL(k_band_form_t, dim3(nb), dim3(256), (size_t)b->form_R * W * kDB * 8, s, b->rowptr, b->colind, b->vals,
                       b->t_rowptr, b->t_colind, b->t_vals, (int)b->m, (int)b->mpad, W, delta, b->Mb, b->form_R);
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
  int32_t pivot = 0;
  const int rc = factor_end(b, &b->info.last_form_ms, &b->info.last_chol_ms, &b->info.regularized_pivots, &pivot);
  if (rc >= 0 && info)  // (first non-positive pivot, 1-based, in the CALLER's row numbering)
    *info = pivot > 0 && b->reordered && pivot <= (int32_t)b->m ? b->rperm_host[pivot - 1] + 1 : pivot;
  return rc;
}

int fpsq_band_solve_two_mixed(fpsq_band b, const double* rhs1, const double* rhs2, double* p1, double* q1, double* p2,
                              double* q2) {
  if (int rc = solve_begin(b, true, rhs1, rhs2, p1, q1, p2, q2)) return rc;
  hipStream_t s = b->stream;
  // r = [A g, -c]:  q1 = M^-1 A g,  q2 = -M^-1 c;  then p1 = g - A'q1, p2 = -A'q2   
  hipLaunchKernelGGL(k_dense_pack2, dim3((unsigned)((b->n + 255) / 256)), dim3(256), 0, s, b->in_a, 1.0,
                     (const double*)nullptr, 0.0, b->xn, (int)b->n, (int)b->n);
  hipLaunchKernelGGL(k_csr_mv2, dim3((unsigned)((b->m + 255) / 256)), dim3(256), 0, s, b->rowptr, b->colind, b->vals, b->xn,
                     b->ym, (int)b->m);
  const double* cperm = b->in_b;
  if (b->reordered) {
    hipLaunchKernelGGL(k_gather_d, dim3((unsigned)((b->m + 255) / 256)), dim3(256), 0, s, b->in_b, b->rperm, b->in_bp, b->m);
    cperm = b->in_bp;
  }
  hipLaunchKernelGGL(k_band_rhs, dim3((unsigned)((b->mpad + 255) / 256)), dim3(256), 0, s, b->ym, 0, cperm, -1.0, b->r2,
                     (int)b->m, (int)b->mpad, 0);
  return band_finish(b, nullptr, p1, q1, p2, q2);
}

int fpsq_band_solve_two_least_squares(fpsq_band b, const double* rhs1, const double* rhs2, double* p1, double* q1,
                                      double* p2, double* q2) {
  if (int rc = solve_begin(b, false, rhs1, rhs2, p1, q1, p2, q2)) return rc;
  hipStream_t s = b->stream;
  hipLaunchKernelGGL(k_dense_pack2, dim3((unsigned)((b->n + 255) / 256)), dim3(256), 0, s, b->in_a, 1.0, b->in_b, 1.0, b->xn,
                     (int)b->n, (int)b->n);
  hipLaunchKernelGGL(k_csr_mv2, dim3((unsigned)((b->m + 255) / 256)), dim3(256), 0, s, b->rowptr, b->colind, b->vals, b->xn,
                     b->ym, (int)b->m);
  hipLaunchKernelGGL(k_band_rhs, dim3((unsigned)((b->mpad + 255) / 256)), dim3(256), 0, s, b->ym, 0, (const double*)nullptr,
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
  double* keep = b->o_q2;
  if (qp->sparse_q) {
#define BQ_PACK_SQ(HP)                                                                                                   \
  hipLaunchKernelGGL((k_bq_pack_sq<LG, HP>), dim3(qp->gridR), dim3(256), 0, s, qp->r_rowptr, qp->r_colind, qp->r_vals, x, \
                     qp->q, qp->d, b->xn, qp->partF, n)
    WITH_LANE_GROUP(qp->lgR, if (hp) BQ_PACK_SQ(true); else BQ_PACK_SQ(false);)
#undef BQ_PACK_SQ
  } else if (!qp->gather_g) {
    if (hp)
      hipLaunchKernelGGL(k_bq_pack<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, qp->q, qp->d, b->xn, n);
    else
      hipLaunchKernelGGL(k_bq_pack<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, qp->q, qp->d, b->xn, n);
  }
#define BQ_PROLOGUE(HP, GM)                                                                                              \
  hipLaunchKernelGGL((k_bq_prologue<LG, HP, GM>), dim3(qp->gridP), dim3(256), 0, s, b->rowptr, b->colind, b->vals, b->xn, x, \
                     qp->q, qp->d, qp->bp, b->r2, keep, qp->partP, m, mpad, n)
  WITH_LANE_GROUP(qp->lgA, if (hp) {
    if (qp->gather_g) BQ_PROLOGUE(true, true);
    else BQ_PROLOGUE(true, false);
  } else {
    if (qp->gather_g) BQ_PROLOGUE(false, true);
    else BQ_PROLOGUE(false, false);
  })
#undef BQ_PROLOGUE
  band_solve(b);
#define BQ_EPILOGUE(HP)                                                                                                   \
  hipLaunchKernelGGL((k_bq_epilogue<LG, HP>), dim3(qp->gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals, b->r2,   \
                     keep, b->reordered ? b->rperm : (const int32_t*)nullptr, x, xk, qp->q, qp->d, sigma, rho, eta, out, gs, \
                     ys, qp->partE, n, m)
#define BQ_EPILOGUE_SQ(HP)                                                                                                 \
  hipLaunchKernelGGL((k_bq_epilogue_sq<LG, HP>), dim3(qp->gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals, b->r2, \
                     keep, b->reordered ? b->rperm : (const int32_t*)nullptr, xk, qp->q, b->xn, sigma, rho, eta, out, gs, ys, \
                     qp->tv, qp->partE, n, m)
  if (!qp->sparse_q) {
    WITH_LANE_GROUP(qp->lgT, if (hp) BQ_EPILOGUE(true); else BQ_EPILOGUE(false);)
    return;
  }
  WITH_LANE_GROUP(qp->lgT, if (hp) BQ_EPILOGUE_SQ(true); else BQ_EPILOGUE_SQ(false);)
  if (out) {  // out -= R p2 (objgrad) resp. R Ptv (hprod): the rows of tv are complete only now
    WITH_LANE_GROUP(qp->lgR, hipLaunchKernelGGL(k_bq_jacmul<LG>, dim3(qp->gridR), dim3(256), 0, s, qp->r_rowptr, qp->r_colind,
                                                qp->r_vals, (const int32_t*)nullptr, (const int32_t*)nullptr, -1.0, qp->tv, 1.0,
                                                out, n))
  }
#undef BQ_EPILOGUE
#undef BQ_EPILOGUE_SQ
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
  if (hipMalloc((void**)&qp->q, nb8) != hipSuccess || hipMalloc((void**)&qp->d, nb8) != hipSuccess ||
      hipMalloc((void**)&qp->bp, mb8) != hipSuccess || hipMalloc((void**)&qp->partP, (size_t)qp->gridP * 16) != hipSuccess ||
      hipMalloc((void**)&qp->partE, (size_t)qp->gridE * 16) != hipSuccess ||
      hipMemcpy(qp->q, qdiag, nb8, hipMemcpyDefault) != hipSuccess || hipMemcpy(qp->d, d, nb8, hipMemcpyDefault) != hipSuccess ||
      hipMemcpy(qp->bp, bs.data(), mb8, hipMemcpyHostToDevice) != hipSuccess) {
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
  // and the split Q = diag(q) + R
  std::vector<int32_t> rp((size_t)n + 1);
  CHK(b, hipMemcpy(rp.data(), q_rowptr, ((size_t)n + 1) * 4, hipMemcpyDefault));
  if (rp[0] != 0) return bad("rowptr[0] must be 0");
  for (int64_t i = 0; i < n; ++i)
    if (rp[i + 1] < rp[i]) return bad("rowptr decreases at row " + std::to_string(i));
  const size_t nnz = (size_t)rp[n];
  if (nnz && (!q_colind || !q_vals)) return FPSQ_ERR_ARG;
  std::vector<int32_t> ci(nnz);
  std::vector<double> va(nnz);
  if (nnz) {
    CHK(b, hipMemcpy(ci.data(), q_colind, nnz * 4, hipMemcpyDefault));
    CHK(b, hipMemcpy(va.data(), q_vals, nnz * 8, hipMemcpyDefault));
  }
  std::vector<std::pair<int32_t, double>> ent(nnz);  // every row sorted by column
  for (int64_t i = 0; i < n; ++i) {
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
      if (ci[k] < 0 || ci[k] >= n)
        return bad("column " + std::to_string(ci[k]) + " of row " + std::to_string(i) + " is out of range");
      ent[k] = {ci[k], va[k]};
    }
    std::sort(ent.begin() + rp[i], ent.begin() + rp[i + 1],
              [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& c) { return a.first < c.first; });
    for (int32_t k = rp[i] + 1; k < rp[i + 1]; ++k)
      if (ent[k].first == ent[k - 1].first)
        return bad("duplicate entry (" + std::to_string(i) + ", " + std::to_string(ent[k].first) + ")");
  }
  std::vector<double> qd((size_t)n, 0.0), rv;
  std::vector<int32_t> rrp((size_t)n + 1, 0), rci;
  rv.reserve(nnz);
  rci.reserve(nnz);
  for (int64_t i = 0; i < n; ++i) {
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
      const int32_t j = ent[k].first;
      if (j == i) {
        qd[i] = ent[k].second;
        continue;
      }
      const auto lo = ent.begin() + rp[j], hi = ent.begin() + rp[j + 1];
      const auto it = std::lower_bound(lo, hi, (int32_t)i,
                                       [](const std::pair<int32_t, double>& a, int32_t col) { return a.first < col; });
      if (it == hi || it->first != i)
        return bad("the pattern is not symmetric: (" + std::to_string(i) + ", " + std::to_string(j) + ") has no transpose");
      if (!(it->second == ent[k].second))
        return bad("the values are not symmetric: Q(" + std::to_string(i) + ", " + std::to_string(j) + ") != Q(" +
                   std::to_string(j) + ", " + std::to_string(i) + ")");
      rci.push_back(j);
      rv.push_back(ent[k].second);
    }
    rrp[i + 1] = (int32_t)rci.size();
  }
  fpsq_band_qp qp = nullptr;
  if (int rc = fpsq_band_qp_create(b, qd.data(), d, bvec, &qp)) return rc;
  const size_t rnz = rci.size();
  qp->sparse_q = true;
  qp->gather_g = false;  // (FPSQ_BAND_QP_G has no meaning here: g needs a product with R)
  qp->lgR = lane_group((int64_t)rnz, n);
  qp->gridR = bq_grid(n, qp->lgR);
  if (hipMalloc((void**)&qp->r_rowptr, ((size_t)n + 1) * 4) != hipSuccess ||
      hipMalloc((void**)&qp->r_colind, std::max<size_t>(rnz, 1) * 4) != hipSuccess ||
      hipMalloc((void**)&qp->r_vals, std::max<size_t>(rnz, 1) * 8) != hipSuccess ||
      hipMalloc((void**)&qp->tv, (size_t)n * 8) != hipSuccess ||
      hipMalloc((void**)&qp->partF, (size_t)qp->gridR * 8) != hipSuccess ||
      hipMemcpy(qp->r_rowptr, rrp.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (rnz && (hipMemcpy(qp->r_colind, rci.data(), rnz * 4, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(qp->r_vals, rv.data(), rnz * 8, hipMemcpyHostToDevice) != hipSuccess))) {
    b->err = "band_qp_create_csr: cannot allocate or fill the objective Hessian";
    fpsq_band_qp_destroy(qp);
    return FPSQ_ERR_HIP;
  }
  *out = qp;
  return FPSQ_OK;
}

int fpsq_band_qp_destroy(fpsq_band_qp qp) {
  if (!qp) return FPSQ_ERR_ARG;
  for (void* p : {(void*)qp->q, (void*)qp->d, (void*)qp->bp, (void*)qp->partP, (void*)qp->partE, (void*)qp->r_rowptr,
                  (void*)qp->r_colind, (void*)qp->r_vals, (void*)qp->tv, (void*)qp->partF})
    if (p) hipFree(p);
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
  const double *dx = nullptr, *dxk = nullptr;
  if (int rc = arg_in(b, x, b->in_a, n, &dx)) return rc;
  if (int rc = arg_in(b, eta > 0.0 ? xk : nullptr, b->in_b, n, &dxk)) return rc;
  double *dgx = arg_out(b, gx, b->o_p1), *dgs = arg_out(b, gs, b->o_p2), *dys = arg_out(b, ys, b->o_q1);
  bq_launches(b, qp, false, dx, dxk, sigma, rho, eta, dgx, dgs, dys);
  if (qp->sparse_q)
    hipLaunchKernelGGL(k_bq_phi_sq, dim3(1), dim3(256), 0, b->stream, qp->partF, qp->gridR, qp->partP, qp->gridP, qp->partE,
                       qp->gridE, rho, eta, b->scal);
  else
    hipLaunchKernelGGL(k_bq_phi, dim3(1), dim3(256), 0, b->stream, qp->partP, qp->gridP, qp->partE, qp->gridE, rho, eta, b->scal);
  if (int rc = arg_back(b, gx, dgx, n)) return rc;
  if (int rc = arg_back(b, gs, dgs, n)) return rc;
  if (int rc = arg_back(b, ys, dys, m)) return rc;
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
  const double* dv = nullptr;
  if (int rc = arg_in(b, v, b->in_a, n, &dv)) return rc;
  double* dHv = arg_out(b, Hv, b->o_p1);
  bq_launches(b, qp, true, dv, nullptr, sigma, rho, eta, dHv, nullptr, nullptr);
  if (int rc = arg_back(b, Hv, dHv, n)) return rc;
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
  const double* dx = nullptr;
  if (int rc = arg_in(b, x, trans ? b->in_b : b->in_a, nx, &dx)) return rc;
  double* dy = arg_out(b, y, trans ? b->o_p1 : b->o_q1);
  if (dy != y && beta != 0.0) CHK(b, hipMemcpyAsync(dy, y, ny * 8, hipMemcpyDefault, s));
  const int32_t* perm = b->reordered ? b->rperm : nullptr;
  const int lg = lane_group(b->nnz, (int64_t)ny);
  if (trans) {
    WITH_LANE_GROUP(lg, hipLaunchKernelGGL(k_bq_jacmul<LG>, dim3(bq_grid(b->n, lg)), dim3(256), 0, s, b->t_rowptr, b->t_colind,
                                           b->t_vals, perm, (const int32_t*)nullptr, alpha, dx, beta, dy, (int)b->n))
  } else {
    WITH_LANE_GROUP(lg, hipLaunchKernelGGL(k_bq_jacmul<LG>, dim3(bq_grid(b->m, lg)), dim3(256), 0, s, b->rowptr, b->colind,
                                           b->vals, (const int32_t*)nullptr, perm, alpha, dx, beta, dy, (int)b->m))
  }
  if (int rc = arg_back(b, y, dy, ny)) return rc;
  CHK(b, hipStreamSynchronize(s));
  return FPSQ_OK;
}
}  // extern "C"

// ------------------------------------------- block entries: a (k, n) block of vectors per call, 8 vectors per pass of the factor

namespace {
// One side of a block argument: in place when it lives on the handle's GPU, else through staging buffer `slot` (len doubles
// per vector), a tile at a time
struct BlockArg {
  double* base = nullptr;
  size_t len = 0;
  bool dev = false;
  double* stage = nullptr;
  double* tile(int v0) const { return !base ? nullptr : dev ? base + (size_t)v0 * len : stage; }
};

int blk_arg(fpsq_band b, const double* p, size_t len, int slot, BlockArg* a) {
  a->base = const_cast<double*>(p);
  a->len = len;
  if (!p) return FPSQ_OK;
  a->dev = on_device(b, p);
  if (!a->dev) {
    if (!b->blk_stage[slot] && dalloc(b, &b->blk_stage[slot], len * kBlkVec)) return FPSQ_ERR_HIP;
    a->stage = b->blk_stage[slot];
  }
  return FPSQ_OK;
}

// the tile's input as the kernels read it / the copy back of a staged output tile
int blk_in(fpsq_band b, const BlockArg& a, int v0, int kt, const double** out) {
  *out = a.tile(v0);
  if (a.base && !a.dev)
    CHK(b, hipMemcpyAsync(a.stage, a.base + (size_t)v0 * a.len, (size_t)kt * a.len * 8, hipMemcpyDefault, b->stream));
  return FPSQ_OK;
}

int blk_back(fpsq_band b, const BlockArg& a, int v0, int kt) {
  if (a.base && !a.dev)
    CHK(b, hipMemcpyAsync(a.base + (size_t)v0 * a.len, a.stage, (size_t)kt * a.len * 8, hipMemcpyDefault, b->stream));
  return FPSQ_OK;
}

// the buffers a block call needs: the sweeps' own and the tiles around them
int blk_setup(fpsq_band b, bool keep, bool tv) {
  if (int rc = chain16_setup(b)) return rc;
  if (!b->blk_xg && dalloc(b, &b->blk_xg, (size_t)b->n * kBlkCols)) return FPSQ_ERR_HIP;
  if (keep && !b->blk_keep && dalloc(b, &b->blk_keep, (size_t)b->mpad * kBlkVec)) return FPSQ_ERR_HIP;
  if (tv && !b->blk_tv && dalloc(b, &b->blk_tv, (size_t)b->n * kBlkVec)) return FPSQ_ERR_HIP;
  return FPSQ_OK;
}

// A xg into the sweeps' layout, then the two sweeps: the tile's solutions end up in b->r16
void blk_solve_tile(fpsq_band b, int lgA, double* keep) {
  WITH_LANE_GROUP(lgA, hipLaunchKernelGGL(k_bqb_prologue<LG>, dim3(bq_grid(b->mpad, lgA)), dim3(256), 0, b->stream, b->rowptr,
                                          b->colind, b->vals, b->blk_xg, b->r16, keep, (int)b->m, (int)b->mpad))
  chain_sweeps16(b, b->Mb, b->band_w, b->chain_safe, b->chain_bw);
}

// end of a block call: eval_end with the text of a block sweep's expired wait
int blk_end(fpsq_band b) {
  const int rc = eval_end(b, 0, &b->info.last_solve_ms);
  if (rc == FPSQ_ERR_TIMEOUT)
    b->err = "block triangular sweep: a block's solution did not arrive (bounded wait expired); the single-vector entries "
             "do not use this kernel";
  return rc;
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
  BlockArg a1, a2, o1, oq1, o2, oq2;
  if (blk_arg(b, rhs1, n, 0, &a1) || blk_arg(b, rhs2, n, 1, &a2) || blk_arg(b, p1, n, 2, &o1) || blk_arg(b, p2, n, 3, &o2) ||
      blk_arg(b, q1, m, 4, &oq1) || blk_arg(b, q2, m, 5, &oq2))
    return FPSQ_ERR_HIP;
  const int lgA = lane_group(b->nnz, b->m), lgT = lane_group(b->nnz, b->n);
  const int32_t* rperm = b->reordered ? b->rperm : nullptr;
  for (int v0 = 0; v0 < k; v0 += kBlkVec) {
    const int kt = std::min<int>(kBlkVec, k - v0);
    const double *d1 = nullptr, *d2 = nullptr;
    if (int rc = blk_in(b, a1, v0, kt, &d1)) return rc;
    if (int rc = blk_in(b, a2, v0, kt, &d2)) return rc;
    hipLaunchKernelGGL(k_bqb_pack<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, d1, d2,
                       (const double*)nullptr, b->blk_xg, (int)n, kt);
    blk_solve_tile(b, lgA, nullptr);
    WITH_LANE_GROUP(lgT, hipLaunchKernelGGL((k_bqb_epilogue<LG, 2>), dim3(bq_grid(b->n, lgT)), dim3(256), 0, b->stream,
                                            b->t_rowptr, b->t_colind, b->t_vals, b->r16, (const double*)nullptr, rperm,
                                            (const double*)nullptr, b->blk_xg, 0.0, 0.0, 0.0, o1.tile(v0), o2.tile(v0),
                                            oq1.tile(v0), oq2.tile(v0), (double*)nullptr, (int)n, (int)m, kt))
    for (const BlockArg* o : {&o1, &o2, &oq1, &oq2})
      if (int rc = blk_back(b, *o, v0, kt)) return rc;
  }
  return blk_end(b);
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
  BlockArg av, ah;
  if (blk_arg(b, V, n, 0, &av) || blk_arg(b, HV, n, 2, &ah)) return FPSQ_ERR_HIP;
  const int32_t* rperm = b->reordered ? b->rperm : nullptr;
  hipStream_t s = b->stream;
  for (int v0 = 0; v0 < k; v0 += kBlkVec) {
    const int kt = std::min<int>(kBlkVec, k - v0);
    const double* dv = nullptr;
    if (int rc = blk_in(b, av, v0, kt, &dv)) return rc;
    double* dh = ah.tile(v0);
    if (qp->sparse_q) {
      WITH_LANE_GROUP(qp->lgR, hipLaunchKernelGGL(k_bqb_pack_sq<LG>, dim3(qp->gridR), dim3(256), 0, s, qp->r_rowptr,
                                                  qp->r_colind, qp->r_vals, dv, qp->q, b->blk_xg, (int)n, kt))
    } else {
      hipLaunchKernelGGL(k_bqb_pack<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dv, (const double*)nullptr, qp->q,
                         b->blk_xg, (int)n, kt);
    }
    blk_solve_tile(b, qp->lgA, b->blk_keep);
#define BQB_EPILOGUE(MODE)                                                                                                   \
  hipLaunchKernelGGL((k_bqb_epilogue<LG, MODE>), dim3(qp->gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals, b->r16, \
                     b->blk_keep, rperm, qp->q, b->blk_xg, sigma, rho, eta, dh, (double*)nullptr, (double*)nullptr,           \
                     (double*)nullptr, b->blk_tv, (int)n, (int)b->m, kt)
    if (qp->sparse_q) {
      WITH_LANE_GROUP(qp->lgT, BQB_EPILOGUE(1))
      WITH_LANE_GROUP(qp->lgR, hipLaunchKernelGGL(k_bqb_rsub<LG>, dim3(qp->gridR), dim3(256), 0, s, qp->r_rowptr, qp->r_colind,
                                                  qp->r_vals, b->blk_tv, dh, (int)n, kt))
    } else {
      WITH_LANE_GROUP(qp->lgT, BQB_EPILOGUE(0))
    }
#undef BQB_EPILOGUE
    if (int rc = blk_back(b, ah, v0, kt)) return rc;
  }
  return blk_end(b);
}
}  // extern "C"
