// fpsq_dense.hip -- host side of the dense-block direct back-end (C ABI: include/fpsq.h, "dense" section).
#include "fpsq_dense.hip.h"

using namespace fpsq;
using namespace fpsq_direct;

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
  hipLaunchKernelGGL(k_dense_finish_p, grid256(d->n), dim3(256), 0, s, d->part, d->nchunk,
                     (int)d->npad, (int)d->n, a0, a1, d->o_p1, d->o_p2);
  hipLaunchKernelGGL(k_dense_unpack2, grid256(d->m), dim3(256), 0, s, d->r2, d->o_q1, d->o_q2,
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
  hipLaunchKernelGGL(k_dense_diag, grid256(d->mpad), dim3(256), 0, s, d->M, ld, (int)d->m, (int)d->mpad,
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
  hipLaunchKernelGGL(k_dense_pack2, grid256(d->npad), dim3(256), 0, s, d->in_a, 1.0,
                     (const double*)nullptr, 0.0, d->x2, (int)d->n, (int)d->npad);
  hipLaunchKernelGGL(k_dense_gemv<2>, dim3((unsigned)((d->mpad + 3) / 4)), dim3(256), 0, s, d->A, (int)d->npad,
                     (int)d->mpad, (int)d->npad, d->x2, 1.0, (const double*)nullptr, 0.0, d->y2);
  hipLaunchKernelGGL(k_dense_unpack2, grid256(d->mpad), dim3(256), 0, s, d->y2, d->o_q1, d->o_q2,
                     (int)d->mpad);
  hipLaunchKernelGGL(k_dense_pack2, grid256(d->mpad), dim3(256), 0, s, d->o_q1, 1.0, d->in_b, -1.0,
                     d->r2, (int)d->m, (int)d->mpad);
  dense_sweeps(d);
  return dense_finish(d, d->in_a, nullptr, p1, q1, p2, q2);
}

int fpsq_dense_solve_two_least_squares(fpsq_dense d, const double* rhs1, const double* rhs2, double* p1, double* q1,
                                       double* p2, double* q2) {
  if (int rc = solve_begin(d, false, rhs1, rhs2, p1, q1, p2, q2)) return rc;
  hipStream_t s = d->stream;
  hipLaunchKernelGGL(k_dense_pack2, grid256(d->npad), dim3(256), 0, s, d->in_a, 1.0, d->in_b, 1.0,
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
