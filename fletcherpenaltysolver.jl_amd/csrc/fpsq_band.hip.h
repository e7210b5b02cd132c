// fpsq_band.hip.h -- kernels of the banded direct back-end alone (fpsq_band.hip): formation of M = A A' + delta I as a
// block band (k_band_form*), the CSR products and vector kernels around the M-solves (k_csr_mv2, k_gather_d, k_band_rhs,
// k_band_finish), the device-resident eq-QP evaluations (k_bq_*) and their block forms (k_bqb_*).
#pragma once
#include "fpsq_direct.hip.h"

namespace fpsq {

// ---- sparse direct path (fpsq_band): M = A A' + delta I of a BANDED sparse Jacobian as a block band
// One workgroup per 128-row block I.  For each of its rows i in turn: scatter the row into a dense LDS window over its
// column span, then every thread takes rows j <= i of the band (blocks I - bw .. I) and gathers its dot product with
// row i from the window (columns outside the window contribute nothing); M(i, j) goes to block (I, j / 128).
// (A wave per band row with unit-stride loads was measured slower -- 114 against 87 ms at the headline size: the loop
// over the band rows then is a chain of dependent loads, whereas 256 threads walking 256 rows keep 256 streams in flight.)
// Deterministic (fixed summation order, no atomics).  rowspan[i] = {first column, last column} of row i.
__global__ __launch_bounds__(256) void k_band_form(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                   const double* __restrict__ vals, const int2* __restrict__ rowspan,
                                                   int m, int mpad, int band_w, double delta, double* Mb, int span) {
  extern __shared__ __attribute__((aligned(16))) double win[];  // two windows of `span` doubles: rows i and i + 1
  const int I = blockIdx.x, tid = threadIdx.x;
  for (int k = tid; k < 2 * span; k += 256) win[k] = 0.0;
  __syncthreads();
  const int i0 = I * kDB;
  const int bw = band_w - 1;
  const int jlo = max(0, I - bw) * kDB;
  // TWO rows of the block per pass: every entry of a band row that is loaded serves both dot products (the band rows
  // are re-read from L2 once per pass: 64 instead of 128 times)
  for (int ii = 0; ii < kDB; ii += 2) {
    const int i = i0 + ii;
    double* Mrow0 = Mb + ((size_t)I * band_w) * kDB * kDB + (size_t)ii * kDB;  // row ii of block (I, I - bw)
    double* Mrow1 = Mrow0 + kDB;
    if (i >= m) {  // padding: identity
      if (tid == 0 && i < mpad) Mrow0[(size_t)bw * kDB * kDB + ii] = 1.0;
      if (tid == 0 && i + 1 < mpad) Mrow1[(size_t)bw * kDB * kDB + ii + 1] = 1.0;
      continue;
    }
    const bool two = i + 1 < m;
    const int s0 = rowptr[i], e0 = rowptr[i + 1], e1 = two ? rowptr[i + 2] : e0;
    const int2 sp0 = rowspan[i];
    const int2 sp1 = two ? rowspan[i + 1] : int2{1, 0};  // (an empty span: nothing matches)
    for (int k = s0 + tid; k < e0; k += 256) win[colind[k] - sp0.x] = vals[k];
    for (int k = e0 + tid; k < e1; k += 256) win[span + colind[k] - sp1.x] = vals[k];
    __syncthreads();
    for (int j = jlo + tid; j <= i + 1 && j < m; j += 256) {
      const int js = rowptr[j], je = rowptr[j + 1];
      double a0 = 0.0, a1 = 0.0;
      for (int k = js; k < je; ++k) {
        const int c = colind[k];
        const double v = vals[k];
        if (c >= sp0.x && c <= sp0.y) a0 += v * win[c - sp0.x];
        if (c >= sp1.x && c <= sp1.y) a1 += v * win[span + c - sp1.x];
      }
      const size_t off = (size_t)((j >> 7) - I + bw) * kDB * kDB + (j & 127);
      if (j <= i) Mrow0[off] = j == i ? a0 + delta : a0;
      if (two) Mrow1[off] = j == i + 1 ? a1 + delta : a1;  // (j <= i + 1 by the loop bound)
    }
    if (!two && i + 1 < mpad && tid == 0) Mrow1[(size_t)bw * kDB * kDB + ii + 1] = 1.0;  // first padding row
    __syncthreads();
    for (int k = s0 + tid; k < e0; k += 256) win[colind[k] - sp0.x] = 0.0;
    for (int k = e0 + tid; k < e1; k += 256) win[span + colind[k] - sp1.x] = 0.0;
    __syncthreads();
  }
}

// The same band by COLUMNS of A (the default when A has no duplicate entries): M(i, :) = sum over the entries (i, k) of
// row i of a_ik * A(:, k), the column read from the transposed structure.  Only structurally non-zero products are
// formed -- nnz(A) * (entries per column) of them, 1e8 at the headline size against the 1.6e10 gather-FMAs of the
// row-pair scheme above (61 ms there).  One workgroup per 128-row block, R rows of it per pass, one group of G = 256 / R
// lanes per row with a dense accumulator row of W * 128 doubles in LDS (columns (I - bw) * 128 ...): the lanes of a
// group take the entries of ONE column of A (distinct rows j: no two lanes touch the same accumulator), the entries
// (i, k) of the row are taken in CSR order, four columns' loads in flight -- so every M(i, j) is summed in a fixed order,
// no atomics.  The accumulator rows are then written out whole (zeros included) and cleared.
__global__ __launch_bounds__(256) void k_band_form_t(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                     const double* __restrict__ vals, const int32_t* __restrict__ t_rowptr,
                                                     const int32_t* __restrict__ t_rowind, const double* __restrict__ t_vals,
                                                     int m, int mpad, int band_w, double delta, double* Mb, int R) {
  extern __shared__ __attribute__((aligned(16))) double win[];  // R accumulator rows of band_w * 128
  const int I = blockIdx.x, tid = threadIdx.x;
  const int G = 256 / R, g = tid / G, gl = tid % G;
  const int roww = band_w * kDB;
  const int base = (I - (band_w - 1)) * kDB;  // global column of accumulator entry 0 (may be negative: never touched)
  for (int k = tid; k < R * roww; k += 256) win[k] = 0.0;
  __syncthreads();
  double* acc = win + (size_t)g * roww - base;  // acc[j], j a global row index of A = column of M
  for (int pass = 0; pass < kDB; pass += R) {
    const int i = I * kDB + pass + g;
    if (i < m) {
      const int s = rowptr[i], e = rowptr[i + 1];
      for (int t = s; t < e; t += 4) {
        int us[4], ue[4], j[4];
        double a[4], v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool ok = t + q < e;
          const int k = colind[ok ? t + q : s];
          a[q] = ok ? vals[t + q] : 0.0;
          us[q] = t_rowptr[k];
          ue[q] = ok ? t_rowptr[k + 1] : us[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int u = us[q] + gl;
          const bool ok = u < ue[q];
          j[q] = ok ? t_rowind[u] : INT32_MAX;
          v[q] = ok ? t_vals[u] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (j[q] <= i) acc[j[q]] += a[q] * v[q];
          for (int u = us[q] + gl + G; u < ue[q]; u += G) {  // columns longer than the group
            const int jj = t_rowind[u];
            if (jj <= i) acc[jj] += a[q] * t_vals[u];
          }
        }
      }
      if (gl == 0) acc[i] += delta;
    } else if (i < mpad && gl == 0) {
      acc[i] = 1.0;  // padding: identity
    }
    __syncthreads();
    for (int idx = tid; idx < R * roww; idx += 256) {
      const int r = idx / roww, e = idx - r * roww;
      Mb[((size_t)I * band_w + (e >> 7)) * kDB * kDB + (size_t)(pass + r) * kDB + (e & 127)] = win[idx];
      win[idx] = 0.0;
    }
    __syncthreads();
  }
}

// y[r][0..1] = sum_k vals[k] x[colind[k]][0..1] over row r of a CSR matrix (two interleaved right-hand sides); one
// thread per row
__global__ __launch_bounds__(256) void k_csr_mv2(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                 const double* __restrict__ vals, const double* __restrict__ x, double* y,
                                                 int rows) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  double a0 = 0.0, a1 = 0.0;
  for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    const double v = vals[k];
    const double2 xv = *reinterpret_cast<const double2*>(x + (size_t)colind[k] * 2);
    a0 += v * xv.x;
    a1 += v * xv.y;
  }
  y[(size_t)r * 2] = a0;
  y[(size_t)r * 2 + 1] = a1;
}

__global__ __launch_bounds__(256) void k_gather_d(const double* __restrict__ in, const int32_t* __restrict__ perm,
                                                  double* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = in[perm[i]];
}

// r[i] = {ag[i][0], sb * b[i]} on rows < m, zero on the padding (the right-hand sides of the two M-solves)
__global__ __launch_bounds__(256) void k_band_rhs(const double* __restrict__ ag, int col, const double* b, double sb,
                                                  double* r, int m, int mpad, int both) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= mpad) return;
  const bool in = i < m;
  r[(size_t)i * 2] = in ? ag[(size_t)i * 2] : 0.0;
  r[(size_t)i * 2 + 1] = in ? (both ? ag[(size_t)i * 2 + 1] : sb * b[i]) : 0.0;
  (void)col;
}

// p1 = a0 - atq[.][0];  p2 = (a1 ? a1 : 0) - atq[.][1]
__global__ __launch_bounds__(256) void k_band_finish(const double* __restrict__ atq, const double* a0, const double* a1,
                                                     double* p1, double* p2, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  p1[i] = a0[i] - atq[(size_t)i * 2];
  p2[i] = (a1 ? a1[i] : 0.0) - atq[(size_t)i * 2 + 1];
}

// ---- device-resident equality-QP evaluations on the banded handle (fpsq_band_qp_*): f = 1/2 x' diag(q) x + d'x, c = A x - b.
// An evaluation is [k_bq_pack] -> k_bq_prologue -> the two sweeps -> k_bq_epilogue [-> k_bq_phi]; A and A' are each read once.
// With a sparse symmetric Q = diag(q) + R (fpsq_band_qp_create_csr; R = the off-diagonal part, full-row CSR) it is
// k_bq_pack_sq -> k_bq_prologue -> the two sweeps -> k_bq_epilogue_sq -> k_bq_jacmul on R [-> k_bq_phi_sq]: R is read twice.
// Both product kernels give a GROUP of LG lanes (a power of two <= 64, chosen from the mean row length when the model is
// created) to a row, so that the value / index loads of a row are contiguous across lanes, and walk the row tiles with a
// grid stride (the grid depends on the shape alone).  Sums are formed in a fixed order -- lanes by xor shuffles, waves in
// index order, workgroups in index order by k_bq_phi -- so an evaluation is bitwise repeatable; no floating-point atomics.

// sum of v[i] over the 256 threads of the workgroup, in thread 0 (sh: 4 * N doubles); every thread must call it
template <int N>
__device__ __forceinline__ void bq_block_sum(double (&v)[N], double* sh) {
#pragma unroll
  for (int i = 0; i < N; ++i)
    for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o);
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < N; ++i) sh[(threadIdx.x >> 6) * N + i] = v[i];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 0; i < N; ++i) v[i] = ((sh[i] + sh[N + i]) + sh[2 * N + i]) + sh[3 * N + i];
  __syncthreads();
}

// the two vectors A multiplies, interleaved: objgrad (HP = false) {g = q x + d, x}; hprod (HP = true) {v, q v}
template <bool HP>
__global__ __launch_bounds__(256) void k_bq_pack(const double* __restrict__ x, const double* __restrict__ q,
                                                 const double* __restrict__ d, double* __restrict__ xg, int n) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double xv = x[j], qv = q[j];
  f64x2 o;
  if (HP) o = f64x2{xv, qv * xv};
  else o = f64x2{qv * xv + d[j], xv};
  *reinterpret_cast<f64x2*>(xg + (size_t)j * 2) = o;
}

// The same pair for Q = diag(q) + R, a lane group per row of R: with s = (R x)_j, objgrad {q_j x_j + d_j + s, x_j}, hprod
// {v_j, q_j v_j + s}.  Objgrad only: part[blk] = this workgroup's slice of f = sum_j x_j (1/2 (Q x)_j + d_j).
template <int LG, bool HP>
__global__ __launch_bounds__(256) void k_bq_pack_sq(const int32_t* __restrict__ r_rowptr, const int32_t* __restrict__ r_colind,
                                                    const double* __restrict__ r_vals, const double* __restrict__ x,
                                                    const double* __restrict__ q, const double* __restrict__ d,
                                                    double* __restrict__ xg, double* __restrict__ part, int n) {
  constexpr int RPB = 256 / LG;
  __shared__ double sh[4];
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  double red[1] = {0.0};
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s = 0.0;
    if (j < n) {
      const int e = r_rowptr[j + 1];
      for (int k = r_rowptr[j] + l; k < e; k += LG) s += r_vals[k] * x[r_colind[k]];
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && j < n) {
      const double xv = x[j], qv = q[j];
      f64x2 o;
      if (HP) {
        o = f64x2{xv, qv * xv + s};
      } else {
        const double dv = d[j];
        o = f64x2{qv * xv + dv + s, xv};
        red[0] += xv * (0.5 * (qv * xv + s) + dv);
      }
      *reinterpret_cast<f64x2*>(xg + (size_t)j * 2) = o;
    }
  }
  if (!HP) {
    bq_block_sum(red, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
  }
}

// One pass over the (stored, i.e. row-permuted) CSR of A with two right-hand sides; row p of the stored order is written
// where the sweeps read it, r[p] = {A g, -(A x - b)} (objgrad) or {A v, A (q v)} (hprod), zero on the padding, and keep[p] = c
// resp. A v stays for the epilogue.  GM: the right-hand sides are formed at gather time from x, q, d instead of being read
// from the packed xg.  Objgrad only: part[2 blk] = this workgroup's slice of f = x.(1/2 q x + d), part[2 blk + 1] = of c.c.
template <int LG, bool HP, bool GM>
__global__ __launch_bounds__(256) void k_bq_prologue(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                     const double* __restrict__ vals, const double* __restrict__ xg,
                                                     const double* __restrict__ x, const double* __restrict__ q,
                                                     const double* __restrict__ d, const double* __restrict__ bp,
                                                     double* __restrict__ r, double* __restrict__ keep,
                                                     double* __restrict__ part, int m, int mpad, int n) {
  constexpr int RPB = 256 / LG;
  __shared__ double sh[8];
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  double red[2] = {0.0, 0.0};
  const int ntiles = (mpad + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * RPB + g;
    double a0 = 0.0, a1 = 0.0;
    if (p < m) {
      const int e = rowptr[p + 1];
      for (int k = rowptr[p] + l; k < e; k += LG) {
        const double a = vals[k];
        const int c = colind[k];
        double u0, u1;
        if (GM) {
          const double xv = x[c], qv = q[c];
          u0 = HP ? xv : qv * xv + d[c];
          u1 = HP ? qv * xv : xv;
        } else {
          const f64x2 t = *reinterpret_cast<const f64x2*>(xg + (size_t)c * 2);
          u0 = t.x;
          u1 = t.y;
        }
        a0 += a * u0;
        a1 += a * u1;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) {
      a0 += __shfl_xor(a0, o);
      a1 += __shfl_xor(a1, o);
    }
    if (l == 0 && p < mpad) {  // (a0 = a1 = 0 on the padding rows)
      double r1 = a1, kv = a0;
      if (!HP && p < m) {
        kv = a1 - bp[p];
        r1 = -kv;
        red[1] += kv * kv;
      }
      *reinterpret_cast<f64x2*>(r + (size_t)p * 2) = f64x2{a0, r1};
      keep[p] = kv;
    }
  }
  if (!HP) {
    const int64_t chunk = ((int64_t)n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
      const double xv = x[j];
      red[0] += xv * (0.5 * q[j] * xv + d[j]);
    }
    bq_block_sum(red, sh);
    if (threadIdx.x == 0) {
      part[(size_t)blockIdx.x * 2] = red[0];
      part[(size_t)blockIdx.x * 2 + 1] = red[1];
    }
  }
}

// One pass over the CSR of A' (column indices = stored rows of A) on the three vectors the evaluation needs -- q1, q2 (the
// sweeps' solution y[p] = {q1, q2}, read in the stored order: un-permuted on the fly) and keep (c resp. A v) -- with the row
// epilogue fused in.  Row j, s1 = (A'q1)_j, s2 = (A'q2)_j, s3 = (A'keep)_j:
//   objgrad: gs_j = g_j - s1 - sigma s2, p2_j = -s2, grad_j = gs_j + (sigma - q_j) p2_j + rho s3 + eta (x_j - xk_j);
//            the workgroup also writes its slice of ys = q1 + sigma q2 in the caller's row order (rperm: stored row -> the
//            caller's, null = identity) and leaves part[2 blk] = its slice of c.ys, part[2 blk + 1] = of |x - xk|^2.
//   hprod:   Ptv_j = s1, p2_j = q_j v_j - s2, Hv_j = p2_j - q_j Ptv_j + 2 sigma Ptv_j + rho s3 + eta v_j   (out = Hv).
// out, gs, ys, xk may be null.
// SQ (Q = diag(q) + R): g_j resp. (Q v)_j and x_j resp. v_j come from the packed pair xg that k_bq_pack_sq wrote (x, d unused),
// and tv_j = p2_j (objgrad) resp. Ptv_j (hprod) is left for the launch that subtracts R tv from out; the row's own terms,
// -q_j p2_j resp. -q_j Ptv_j among them, are as above.
template <int LG, bool HP, bool SQ>
__device__ __forceinline__ void bq_epilogue_rows(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                 const double* __restrict__ t_vals, const double* __restrict__ y,
                                                 const double* __restrict__ keep, const int32_t* __restrict__ rperm,
                                                 const double* __restrict__ x, const double* __restrict__ xk,
                                                 const double* __restrict__ q, const double* __restrict__ d,
                                                 const double* __restrict__ xg, double sigma, double rho, double eta,
                                                 double* __restrict__ out, double* __restrict__ gs, double* __restrict__ ys,
                                                 double* __restrict__ tv, double* __restrict__ part, int n, int m) {
  constexpr int RPB = 256 / LG;
  __shared__ double sh[8];
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  double red[2] = {0.0, 0.0};
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (j < n) {
      const int e = t_rowptr[j + 1];
      for (int k = t_rowptr[j] + l; k < e; k += LG) {
        const double a = t_vals[k];
        const int p = t_colind[k];
        const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
        s1 += a * t.x;
        s2 += a * t.y;
        s3 += a * keep[p];
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
      s3 += __shfl_xor(s3, o);
    }
    if (l == 0 && j < n) {
      double xv, qv, u;  // u: g_j (objgrad), (Q v)_j (hprod)
      if (SQ) {
        const f64x2 t = *reinterpret_cast<const f64x2*>(xg + (size_t)j * 2);
        xv = HP ? t.x : t.y;
        qv = q[j];
        u = HP ? t.y : t.x;
        tv[j] = HP ? s1 : -s2;
      } else {
        xv = x[j];
        qv = q[j];
        u = HP ? qv * xv : qv * xv + d[j];
      }
      if (HP) {
        out[j] = (u - s2) - qv * s1 + 2.0 * sigma * s1 + rho * s3 + eta * xv;
      } else {
        const double gsv = u - s1 - sigma * s2, p2 = -s2;
        const double dx = eta > 0.0 ? xv - (xk ? xk[j] : 0.0) : 0.0;
        if (gs) gs[j] = gsv;
        if (out) out[j] = gsv + (sigma - qv) * p2 + rho * s3 + eta * dx;
        red[1] += dx * dx;
      }
    }
  }
  if (!HP) {
    const int64_t chunk = ((int64_t)m + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < m ? lo + chunk : m;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
      const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
      const double yv = t.x + sigma * t.y;
      if (ys) ys[rperm ? rperm[p] : p] = yv;
      red[0] += keep[p] * yv;
    }
    bq_block_sum(red, sh);
    if (threadIdx.x == 0) {
      part[(size_t)blockIdx.x * 2] = red[0];
      part[(size_t)blockIdx.x * 2 + 1] = red[1];
    }
  }
}

template <int LG, bool HP>
__global__ __launch_bounds__(256) void k_bq_epilogue(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                     const double* __restrict__ t_vals, const double* __restrict__ y,
                                                     const double* __restrict__ keep, const int32_t* __restrict__ rperm,
                                                     const double* __restrict__ x, const double* __restrict__ xk,
                                                     const double* __restrict__ q, const double* __restrict__ d, double sigma,
                                                     double rho, double eta, double* __restrict__ out,
                                                     double* __restrict__ gs, double* __restrict__ ys,
                                                     double* __restrict__ part, int n, int m) {
  bq_epilogue_rows<LG, HP, false>(t_rowptr, t_colind, t_vals, y, keep, rperm, x, xk, q, d, nullptr, sigma, rho, eta, out, gs, ys,
                                  nullptr, part, n, m);
}

template <int LG, bool HP>
__global__ __launch_bounds__(256) void k_bq_epilogue_sq(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                        const double* __restrict__ t_vals, const double* __restrict__ y,
                                                        const double* __restrict__ keep, const int32_t* __restrict__ rperm,
                                                        const double* __restrict__ xk, const double* __restrict__ q,
                                                        const double* __restrict__ xg, double sigma, double rho, double eta,
                                                        double* __restrict__ out, double* __restrict__ gs,
                                                        double* __restrict__ ys, double* __restrict__ tv,
                                                        double* __restrict__ part, int n, int m) {
  bq_epilogue_rows<LG, HP, true>(t_rowptr, t_colind, t_vals, y, keep, rperm, nullptr, xk, q, nullptr, xg, sigma, rho, eta, out,
                                 gs, ys, tv, part, n, m);
}

// The scalars of an objgrad from the workgroups' partials, each summed in index order (one workgroup: thread t takes a
// contiguous run, then the fixed tree of bq_block_sum): out = {phi, f, c.c, c.ys, |x - xk|^2},
// phi = f - c.ys + rho/2 c.c + eta/2 |x - xk|^2.
__global__ __launch_bounds__(256) void k_bq_phi(const double* __restrict__ partP, int nP, const double* __restrict__ partE,
                                                int nE, double rho, double eta, double* __restrict__ out) {
  __shared__ double sh[16];
  double red[4] = {0.0, 0.0, 0.0, 0.0};
  const int cp = (nP + 255) / 256, ce = (nE + 255) / 256;
  for (int i = threadIdx.x * cp; i < min(nP, ((int)threadIdx.x + 1) * cp); ++i) {
    red[0] += partP[(size_t)i * 2];
    red[1] += partP[(size_t)i * 2 + 1];
  }
  for (int i = threadIdx.x * ce; i < min(nE, ((int)threadIdx.x + 1) * ce); ++i) {
    red[2] += partE[(size_t)i * 2];
    red[3] += partE[(size_t)i * 2 + 1];
  }
  bq_block_sum(red, sh);
  if (threadIdx.x == 0) {
    double phi = red[0] - red[2];
    phi += 0.5 * rho * red[1];
    phi += 0.5 * eta * red[3];
    out[0] = phi;
    out[1] = red[0];
    out[2] = red[1];
    out[3] = red[2];
    out[4] = red[3];
  }
}

// The same for Q = diag(q) + R: f comes from partF (the nF workgroups of k_bq_pack_sq, one double each), partP[2 i] is not read.
__global__ __launch_bounds__(256) void k_bq_phi_sq(const double* __restrict__ partF, int nF, const double* __restrict__ partP,
                                                   int nP, const double* __restrict__ partE, int nE, double rho, double eta,
                                                   double* __restrict__ out) {
  __shared__ double sh[16];
  double red[4] = {0.0, 0.0, 0.0, 0.0};
  const int cf = (nF + 255) / 256, cp = (nP + 255) / 256, ce = (nE + 255) / 256;
  for (int i = threadIdx.x * cf; i < min(nF, ((int)threadIdx.x + 1) * cf); ++i) red[0] += partF[i];
  for (int i = threadIdx.x * cp; i < min(nP, ((int)threadIdx.x + 1) * cp); ++i) red[1] += partP[(size_t)i * 2 + 1];
  for (int i = threadIdx.x * ce; i < min(nE, ((int)threadIdx.x + 1) * ce); ++i) {
    red[2] += partE[(size_t)i * 2];
    red[3] += partE[(size_t)i * 2 + 1];
  }
  bq_block_sum(red, sh);
  if (threadIdx.x == 0) {
    double phi = red[0] - red[2];
    phi += 0.5 * rho * red[1];
    phi += 0.5 * eta * red[3];
    out[0] = phi;
    out[1] = red[0];
    out[2] = red[1];
    out[3] = red[2];
    out[4] = red[3];
  }
}

// y[o(r)] = alpha sum_k vals[k] x[i(colind[k])] + beta y[o(r)] over the rows of a CSR matrix, a lane group per row;
// in_perm / out_perm (null = identity) translate stored rows of A to the caller's: A x takes out_perm, A' x takes in_perm
template <int LG>
__global__ __launch_bounds__(256) void k_bq_jacmul(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                   const double* __restrict__ vals, const int32_t* __restrict__ in_perm,
                                                   const int32_t* __restrict__ out_perm, double alpha,
                                                   const double* __restrict__ x, double beta, double* y, int rows) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (rows + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r = tile * RPB + g;
    double s = 0.0;
    if (r < rows) {
      const int e = rowptr[r + 1];
      for (int k = rowptr[r] + l; k < e; k += LG) {
        const int c = colind[k];
        s += vals[k] * x[in_perm ? in_perm[c] : c];
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && r < rows) {
      const int o = out_perm ? out_perm[r] : r;
      y[o] = alpha * s + (beta != 0.0 ? beta * y[o] : 0.0);
    }
  }
}

// ---- LONG ROWS of R (fpsq_band_nlp_create_coupled_arrow): a long column coupled to the states owns a row of R = -Wo(ys) with up
// to m entries.  The CSR the lane-group kernels above see holds those rows EMPTY; they are listed behind it in the same index
// and value arrays (entry k of long row i: [ptr[i], ptr[i + 1]), column col[k], value slot k, contributors
// [cptr[k], cptr[k + 1]) as fpsq_coupled.h lists them), and each is summed by ONE WORKGROUP in the manner of bn_lc_sums: the
// threads stride the row, four entries of a thread per trip so that their gathered loads are in flight together, a thread's
// terms in index order, lanes by xor shuffles, waves in index order; no atomics.  A model view without long rows carries a null
// pointer and launches nothing of this.
struct bq_long_rows {
  int cols = 0;                                                   // long columns = workgroups
  const int32_t *ptr = nullptr, *col = nullptr, *lcols = nullptr;  // cols + 1, entries, the columns themselves
  const int32_t *cptr = nullptr, *crow = nullptr;                  // contributor lists (Val(1) sums Wo(q1) from them)
  const double* cw = nullptr;
  const double *rv = nullptr, *wq2 = nullptr, *wc = nullptr;       // -Wo(ys), Wo(q2), Wo(c) on the slots
};

// What row T = lcols[i] lacks behind the launch that walked the other rows of R, by mode:
//   LR_OBJ   behind k_bcn_finish:     out_T += sum_k (Wo(q2)_Tk gs_k + Wo(ys)_Tk p2_k)                      u0 = gs, u1 = p2
//   LR_PACK  behind k_bq_pack_sq<HP>: xg[T].y += sum_k R_Tk v_k   (out = xg)                                 u0 = v
//   LR_HV2   behind k_bq_jacmul on R: out_T -= sum_k R_Tk Ptv_k, and += sum_k Wo(c)_Tk v_k when rho > 0      u0 = v, u1 = Ptv
//   LR_HV1   behind k_bcn_finish_h1:  out_T += sum_k (rho Wo(c)_Tk v_k - R_Tk Ptv_k - Wo(q1)_Tk gs_k)        u0 = v, u1 = Ptv, u2 = gs,
//            Wo(q1) from the contributor lists and the first solve's y[p] = {q1, .}
enum { LR_OBJ = 0, LR_PACK = 1, LR_HV2 = 2, LR_HV1 = 3 };

template <int MODE>
__device__ __forceinline__ double bq_long_row_term(const bq_long_rows& L, int k, const double* __restrict__ u0,
                                                   const double* __restrict__ u1, const double* __restrict__ u2,
                                                   const double* __restrict__ y, double rho) {
  const int c = L.col[k];
  if constexpr (MODE == LR_OBJ) {
    return L.wq2[k] * u0[c] - L.rv[k] * u1[c];
  } else if constexpr (MODE == LR_PACK) {
    return L.rv[k] * u0[c];
  } else if constexpr (MODE == LR_HV2) {
    const double t = -(L.rv[k] * u1[c]);
    return rho > 0.0 ? t + L.wc[k] * u0[c] : t;
  } else {
    double wq1 = 0.0;
    const int ue = L.cptr[k + 1];
    for (int u = L.cptr[k]; u < ue; ++u) wq1 += L.cw[u] * y[(size_t)L.crow[u] * 2];
    return (rho * L.wc[k]) * u0[c] - L.rv[k] * u1[c] - wq1 * u2[c];
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_bq_long_rows(bq_long_rows L, const double* __restrict__ u0, const double* __restrict__ u1,
                                                      const double* __restrict__ u2, const double* __restrict__ y, double rho,
                                                      double* __restrict__ out) {
  __shared__ double sh[4];
  const int i = blockIdx.x;
  double s[1] = {0.0};
  const int e = L.ptr[i + 1];
  int k = L.ptr[i] + threadIdx.x;
  for (; k + 3 * 256 < e; k += 4 * 256) {
    double t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = bq_long_row_term<MODE>(L, k + u * 256, u0, u1, u2, y, rho);
#pragma unroll
    for (int u = 0; u < 4; ++u) s[0] += t[u];
  }
  for (; k < e; k += 256) s[0] += bq_long_row_term<MODE>(L, k, u0, u1, u2, y, rho);
  bq_block_sum(s, sh);
  if (threadIdx.x == 0) {
    const int j = L.lcols[i];
    if constexpr (MODE == LR_PACK)
      out[(size_t)j * 2 + 1] += s[0];
    else
      out[j] += s[0];
  }
}


// ---- block forms of the product kernels (fpsq_band_qp_hprod_block, fpsq_band_solve_two_least_squares_block): a TILE of up
// to kBlkVec vectors, vector v of a block at base + v * len (C-contiguous (k, len)), travels through A, the two sweeps
// (k_trsm_chain16) and A' together, so every index and value of A, A' and R is read once per tile.  Between the kernels the
// tile is interleaved: xg[j][2 v], xg[j][2 v + 1] = the pair A multiplies for vector v (hprod {v, Q v}, solve {rhs1, rhs2}),
// r / y [p][2 v], [p][2 v + 1] = the right-hand sides / solutions of its two M-solves, keep[p][v] = A v, tv[j][v] = Ptv.
// Columns kt <= v < kBlkVec of a short tile are ZERO from the pack on; every column is computed by the same instructions
// in the same order whatever its neighbours hold, sums in a fixed order (lanes by xor shuffles), no atomics.
constexpr int kBlkVec = kBlkCols / 2;

// HP: xg[j] = {V[v][j], q[j] V[v][j]}_v;  else {V[v][j], W[v][j]}_v
template <bool HP>
__global__ __launch_bounds__(256) void k_bqb_pack(const double* __restrict__ V, const double* __restrict__ W,
                                                  const double* __restrict__ q, double* __restrict__ xg, int n, int kt) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double qv = HP ? q[j] : 0.0;
#pragma unroll
  for (int v = 0; v < kBlkVec; ++v) {
    f64x2 o = {0.0, 0.0};
    if (v < kt) {
      const double x = V[(size_t)v * n + j];
      o = f64x2{x, HP ? qv * x : W[(size_t)v * n + j]};
    }
    *reinterpret_cast<f64x2*>(xg + (size_t)j * kBlkCols + 2 * v) = o;
  }
}

// The hprod pair for Q = diag(q) + R, a lane group per row of R: xg[j] = {V[v][j], q[j] V[v][j] + (R V[v])_j}_v
template <int LG>
__global__ __launch_bounds__(256) void k_bqb_pack_sq(const int32_t* __restrict__ r_rowptr, const int32_t* __restrict__ r_colind,
                                                     const double* __restrict__ r_vals, const double* __restrict__ V,
                                                     const double* __restrict__ q, double* __restrict__ xg, int n, int kt) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s[kBlkVec];
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v) s[v] = 0.0;
    if (j < n) {
      const int e = r_rowptr[j + 1];
      for (int k = r_rowptr[j] + l; k < e; k += LG) {
        const double a = r_vals[k];
        const int c = r_colind[k];
#pragma unroll
        for (int v = 0; v < kBlkVec; ++v)
          if (v < kt) s[v] += a * V[(size_t)v * n + c];
      }
    }
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v)
#pragma unroll
      for (int o = LG / 2; o > 0; o >>= 1) s[v] += __shfl_xor(s[v], o);
    if (l == 0 && j < n) {
      const double qv = q[j];
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v) {
        f64x2 o = {0.0, 0.0};
        if (v < kt) {
          const double x = V[(size_t)v * n + j];
          o = f64x2{x, qv * x + s[v]};
        }
        *reinterpret_cast<f64x2*>(xg + (size_t)j * kBlkCols + 2 * v) = o;
      }
    }
  }
}

// One pass over the stored CSR of A for the 16 columns of a tile: r[p] = (A xg)[p] where the sweeps read it (row p of the
// stored order, zero on the padding), keep[p][v] = r[p][2 v] (= A v; null: not kept)
template <int LG>
__global__ __launch_bounds__(256) void k_bqb_prologue(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                      const double* __restrict__ vals, const double* __restrict__ xg,
                                                      double* __restrict__ r, double* __restrict__ keep, int m, int mpad) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (mpad + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * RPB + g;
    double acc[kBlkCols];
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c) acc[c] = 0.0;
    if (p < m) {
      const int e = rowptr[p + 1];
      for (int k = rowptr[p] + l; k < e; k += LG) {
        const double a = vals[k];
        const f64x2* t = reinterpret_cast<const f64x2*>(xg + (size_t)colind[k] * kBlkCols);
#pragma unroll
        for (int v = 0; v < kBlkVec; ++v) {
          const f64x2 u = t[v];
          acc[2 * v] += a * u.x;
          acc[2 * v + 1] += a * u.y;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c)
#pragma unroll
      for (int o = LG / 2; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
    if (l == 0 && p < mpad) {  // (zero on the padding rows)
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v) {
        *reinterpret_cast<f64x2*>(r + (size_t)p * kBlkCols + 2 * v) = f64x2{acc[2 * v], acc[2 * v + 1]};
        if (keep) keep[(size_t)p * kBlkVec + v] = acc[2 * v];
      }
    }
  }
}

// One pass over the CSR of A' for a tile, the row epilogue per column.  Row j, vector v: s1 = (A'q1)_j, s2 = (A'q2)_j with
// y[p] = {q1, q2}_v the sweeps' solution in the stored order, s3 = (A'keep)_j.
//   MODE 0 (hprod, Q = diag(q)), 1 (hprod, Q = diag(q) + R):  Ptv = s1, p2 = (Q v)_j - s2 with {v_j, (Q v)_j} from xg,
//       o1[v][j] = Hv = p2 - q_j Ptv + 2 sigma Ptv + rho s3 + eta v_j;  MODE 1 leaves tv[j][v] = Ptv for k_bqb_rsub.
//   MODE 2 (solve_two_least_squares):  o1[v][j] = p1 = rhs1 - s1, o2[v][j] = p2 = rhs2 - s2 (null: not produced), and the
//       workgroup writes its slice of oq1[v] = q1, oq2[v] = q2 in the caller's row order (rperm: stored row -> the caller's,
//       null = identity; null outputs: not produced).
template <int LG, int MODE>
__global__ __launch_bounds__(256) void k_bqb_epilogue(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                      const double* __restrict__ t_vals, const double* __restrict__ y,
                                                      const double* __restrict__ keep, const int32_t* __restrict__ rperm,
                                                      const double* __restrict__ q, const double* __restrict__ xg, double sigma,
                                                      double rho, double eta, double* __restrict__ o1, double* __restrict__ o2,
                                                      double* __restrict__ oq1, double* __restrict__ oq2,
                                                      double* __restrict__ tv, int n, int m, int kt) {
  constexpr int RPB = 256 / LG;
  constexpr bool HP = MODE != 2;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s12[kBlkCols], s3[kBlkVec];
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c) s12[c] = 0.0;
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v) s3[v] = 0.0;
    if (j < n) {
      const int e = t_rowptr[j + 1];
      for (int k = t_rowptr[j] + l; k < e; k += LG) {
        const double a = t_vals[k];
        const int p = t_colind[k];
        const f64x2* t = reinterpret_cast<const f64x2*>(y + (size_t)p * kBlkCols);
#pragma unroll
        for (int v = 0; v < kBlkVec; ++v) {
          const f64x2 u = t[v];
          s12[2 * v] += a * u.x;
          s12[2 * v + 1] += a * u.y;
        }
        if (HP) {
          const f64x2* kp = reinterpret_cast<const f64x2*>(keep + (size_t)p * kBlkVec);
#pragma unroll
          for (int v = 0; v < kBlkVec / 2; ++v) {
            const f64x2 u = kp[v];
            s3[2 * v] += a * u.x;
            s3[2 * v + 1] += a * u.y;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c)
#pragma unroll
      for (int o = LG / 2; o > 0; o >>= 1) s12[c] += __shfl_xor(s12[c], o);
    if (HP) {
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v)
#pragma unroll
        for (int o = LG / 2; o > 0; o >>= 1) s3[v] += __shfl_xor(s3[v], o);
    }
    if (l == 0 && j < n) {
      const double qv = HP ? q[j] : 0.0;
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v) {
        const f64x2 t = *reinterpret_cast<const f64x2*>(xg + (size_t)j * kBlkCols + 2 * v);
        const double s1 = s12[2 * v], s2 = s12[2 * v + 1];
        if (MODE == 1) tv[(size_t)j * kBlkVec + v] = s1;
        if (v < kt) {
          if (HP) {
            o1[(size_t)v * n + j] = (t.y - s2) - qv * s1 + 2.0 * sigma * s1 + rho * s3[v] + eta * t.x;
          } else {
            if (o1) o1[(size_t)v * n + j] = t.x - s1;
            if (o2) o2[(size_t)v * n + j] = t.y - s2;
          }
        }
      }
    }
  }
  if (MODE == 2 && (oq1 || oq2)) {
    const int64_t chunk = ((int64_t)m + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < m ? lo + chunk : m;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
      const size_t dst = (size_t)(rperm ? rperm[p] : p);
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v) {
        if (v < kt) {
          const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * kBlkCols + 2 * v);
          if (oq1) oq1[(size_t)v * m + dst] = t.x;
          if (oq2) oq2[(size_t)v * m + dst] = t.y;
        }
      }
    }
  }
}

// out[v][j] -= (R tv[.][v])_j for the vectors of a tile, a lane group per row of R (tv: [n][kBlkVec], complete only after the
// A' pass)
template <int LG>
__global__ __launch_bounds__(256) void k_bqb_rsub(const int32_t* __restrict__ r_rowptr, const int32_t* __restrict__ r_colind,
                                                  const double* __restrict__ r_vals, const double* __restrict__ tv, double* out,
                                                  int n, int kt) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s[kBlkVec];
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v) s[v] = 0.0;
    if (j < n) {
      const int e = r_rowptr[j + 1];
      for (int k = r_rowptr[j] + l; k < e; k += LG) {
        const double a = r_vals[k];
        const f64x2* t = reinterpret_cast<const f64x2*>(tv + (size_t)r_colind[k] * kBlkVec);
#pragma unroll
        for (int v = 0; v < kBlkVec / 2; ++v) {
          const f64x2 u = t[v];
          s[2 * v] += a * u.x;
          s[2 * v + 1] += a * u.y;
        }
      }
    }
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v)
#pragma unroll
      for (int o = LG / 2; o > 0; o >>= 1) s[v] += __shfl_xor(s[v], o);
    if (l == 0 && j < n) {
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v)
        if (v < kt) out[(size_t)v * n + j] -= s[v];
    }
  }
}

// ---- objgrad form of the block kernels (fpsq_band_qp_objgrad_block): vector v of a tile is the evaluation at X[v] on the
// model with its linear term replaced by D[v] (null: the model's d) and its right-hand side by Bv[v] (null: the model's b).
// The tile is interleaved as above: xg[j][2 v], [2 v + 1] = {g, x}, r[p][2 v], [2 v + 1] = {A g, -c}, keep[p][v] = c,
// tv[j][v] = p2.  The scalars of a column are summed like those of the single evaluation, per column: lanes by xor shuffles,
// waves in index order (bq_block_sum), the workgroups' partials part[blk][column] in index order by k_bqb_phi.  Columns
// kt <= v < kBlkVec are zero everywhere and their partials are zero.

// xg[j] = {q[j] X[v][j] + d_v[j], X[v][j]}_v
__global__ __launch_bounds__(256) void k_bqb_og_pack(const double* __restrict__ X, const double* __restrict__ D,
                                                     const double* __restrict__ d, const double* __restrict__ q,
                                                     double* __restrict__ xg, int n, int kt) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double qv = q[j], dm = d[j];
#pragma unroll
  for (int v = 0; v < kBlkVec; ++v) {
    f64x2 o = {0.0, 0.0};
    if (v < kt) {
      const double x = X[(size_t)v * n + j];
      const double dv = D ? D[(size_t)v * n + j] : dm;
      o = f64x2{qv * x + dv, x};
    }
    *reinterpret_cast<f64x2*>(xg + (size_t)j * kBlkCols + 2 * v) = o;
  }
}

// The same pair for Q = diag(q) + R, a lane group per row of R: xg[j] = {q[j] X[v][j] + d_v[j] + (R X[v])_j, X[v][j]}_v, and
// part[blk][v] = this workgroup's slice of f_v = sum_j X[v][j] (1/2 (Q X[v])_j + d_v[j])
template <int LG>
__global__ __launch_bounds__(256) void k_bqb_og_pack_sq(const int32_t* __restrict__ r_rowptr,
                                                        const int32_t* __restrict__ r_colind,
                                                        const double* __restrict__ r_vals, const double* __restrict__ X,
                                                        const double* __restrict__ D, const double* __restrict__ d,
                                                        const double* __restrict__ q, double* __restrict__ xg,
                                                        double* __restrict__ part, int n, int kt) {
  constexpr int RPB = 256 / LG;
  __shared__ double sh[4 * kBlkVec];
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  double red[kBlkVec];
#pragma unroll
  for (int v = 0; v < kBlkVec; ++v) red[v] = 0.0;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s[kBlkVec];
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v) s[v] = 0.0;
    if (j < n) {
      const int e = r_rowptr[j + 1];
      for (int k = r_rowptr[j] + l; k < e; k += LG) {
        const double a = r_vals[k];
        const int c = r_colind[k];
#pragma unroll
        for (int v = 0; v < kBlkVec; ++v)
          if (v < kt) s[v] += a * X[(size_t)v * n + c];
      }
    }
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v)
#pragma unroll
      for (int o = LG / 2; o > 0; o >>= 1) s[v] += __shfl_xor(s[v], o);
    if (l == 0 && j < n) {
      const double qv = q[j], dm = d[j];
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v) {
        f64x2 o = {0.0, 0.0};
        if (v < kt) {
          const double x = X[(size_t)v * n + j];
          const double dv = D ? D[(size_t)v * n + j] : dm;
          o = f64x2{qv * x + dv + s[v], x};
          red[v] += x * (0.5 * (qv * x + s[v]) + dv);
        }
        *reinterpret_cast<f64x2*>(xg + (size_t)j * kBlkCols + 2 * v) = o;
      }
    }
  }
  bq_block_sum(red, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v) part[(size_t)blockIdx.x * kBlkVec + v] = red[v];
  }
}

// One pass over the stored CSR of A for the 16 columns of a tile: with c_v[p] = (A X[v])_p - b_v[p], r[p] = {(A g_v)_p,
// -c_v[p]}_v where the sweeps read it and keep[p][v] = c_v[p], all zero on the padding rows.  The model's b (bp) is in the
// stored row order; a caller's Bv is in the caller's and is gathered through rperm (stored row -> the caller's, null =
// identity).  part[blk][v] = {this workgroup's slice of f_v = X[v].(1/2 q X[v] + d_v) (FD: Q = diag(q); else 0: the pack
// kernel has it), of c_v.c_v}.
template <int LG, bool FD>
__global__ __launch_bounds__(256) void k_bqb_og_prologue(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                         const double* __restrict__ vals, const double* __restrict__ xg,
                                                         const double* __restrict__ X, const double* __restrict__ D,
                                                         const double* __restrict__ d, const double* __restrict__ q,
                                                         const double* __restrict__ Bv, const double* __restrict__ bp,
                                                         const int32_t* __restrict__ rperm, double* __restrict__ r,
                                                         double* __restrict__ keep, double* __restrict__ part, int m, int mpad,
                                                         int n, int kt) {
  constexpr int RPB = 256 / LG;
  __shared__ double sh[4 * kBlkCols];
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  double red[kBlkCols];  // [2 v] = f_v, [2 v + 1] = c_v.c_v
#pragma unroll
  for (int c = 0; c < kBlkCols; ++c) red[c] = 0.0;
  const int ntiles = (mpad + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * RPB + g;
    double acc[kBlkCols];
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c) acc[c] = 0.0;
    if (p < m) {
      const int e = rowptr[p + 1];
      for (int k = rowptr[p] + l; k < e; k += LG) {
        const double a = vals[k];
        const f64x2* t = reinterpret_cast<const f64x2*>(xg + (size_t)colind[k] * kBlkCols);
#pragma unroll
        for (int v = 0; v < kBlkVec; ++v) {
          const f64x2 u = t[v];
          acc[2 * v] += a * u.x;
          acc[2 * v + 1] += a * u.y;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c)
#pragma unroll
      for (int o = LG / 2; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
    if (l == 0 && p < mpad) {
      const bool row = p < m;
      const size_t src = row && Bv ? (size_t)(rperm ? rperm[p] : p) : 0;
      const double bm = row && !Bv ? bp[p] : 0.0;
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v) {
        double a0 = 0.0, r1 = 0.0, cv = 0.0;
        if (row && v < kt) {
          a0 = acc[2 * v];
          cv = acc[2 * v + 1] - (Bv ? Bv[(size_t)v * m + src] : bm);
          r1 = -cv;
          red[2 * v + 1] += cv * cv;
        }
        *reinterpret_cast<f64x2*>(r + (size_t)p * kBlkCols + 2 * v) = f64x2{a0, r1};
        keep[(size_t)p * kBlkVec + v] = cv;
      }
    }
  }
  if (FD) {
    const int64_t chunk = ((int64_t)n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
      const double qv = q[j], dm = d[j];
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v) {
        if (v < kt) {
          const double x = X[(size_t)v * n + j];
          const double dv = D ? D[(size_t)v * n + j] : dm;
          red[2 * v] += x * (0.5 * qv * x + dv);
        }
      }
    }
  }
  bq_block_sum(red, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c) part[(size_t)blockIdx.x * kBlkCols + c] = red[c];
  }
}

// One pass over the CSR of A' for a tile with the objgrad row epilogue of bq_epilogue_rows per column.  Row j, vector v, with
// {g, x} from xg, s1 = (A'q1)_j, s2 = (A'q2)_j (y[p] = {q1, q2}_v: the sweeps' solution in the stored order), s3 = (A'c_v)_j:
//   GS[v][j] = gs = g - s1 - sigma s2, p2 = -s2, GX[v][j] = gs + (sigma - q_j) p2 + rho s3 + eta (x - XK[v][j]);
// SQ (Q = diag(q) + R) leaves tv[j][v] = p2 for k_bqb_rsub.  The workgroup also writes its slice of YS[v] = q1 + sigma q2 in
// the caller's row order (rperm) and part[blk][v] = {its slice of c_v.ys_v, of |x - xk|^2 (0 unless eta > 0)}.
// GX, GS, YS, XK may be null (XK: xk = 0).
template <int LG, bool SQ>
__global__ __launch_bounds__(256) void k_bqb_og_epilogue(const int32_t* __restrict__ t_rowptr,
                                                         const int32_t* __restrict__ t_colind,
                                                         const double* __restrict__ t_vals, const double* __restrict__ y,
                                                         const double* __restrict__ keep, const int32_t* __restrict__ rperm,
                                                         const double* __restrict__ q, const double* __restrict__ xg,
                                                         const double* __restrict__ XK, double sigma, double rho, double eta,
                                                         double* __restrict__ GX, double* __restrict__ GS,
                                                         double* __restrict__ YS, double* __restrict__ tv,
                                                         double* __restrict__ part, int n, int m, int kt) {
  constexpr int RPB = 256 / LG;
  __shared__ double sh[4 * kBlkCols];
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  double red[kBlkCols];  // [2 v] = c_v.ys_v, [2 v + 1] = |x - xk|^2
#pragma unroll
  for (int c = 0; c < kBlkCols; ++c) red[c] = 0.0;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s12[kBlkCols], s3[kBlkVec];
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c) s12[c] = 0.0;
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v) s3[v] = 0.0;
    if (j < n) {
      const int e = t_rowptr[j + 1];
      for (int k = t_rowptr[j] + l; k < e; k += LG) {
        const double a = t_vals[k];
        const int p = t_colind[k];
        const f64x2* t = reinterpret_cast<const f64x2*>(y + (size_t)p * kBlkCols);
#pragma unroll
        for (int v = 0; v < kBlkVec; ++v) {
          const f64x2 u = t[v];
          s12[2 * v] += a * u.x;
          s12[2 * v + 1] += a * u.y;
        }
        const f64x2* kp = reinterpret_cast<const f64x2*>(keep + (size_t)p * kBlkVec);
#pragma unroll
        for (int v = 0; v < kBlkVec / 2; ++v) {
          const f64x2 u = kp[v];
          s3[2 * v] += a * u.x;
          s3[2 * v + 1] += a * u.y;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c)
#pragma unroll
      for (int o = LG / 2; o > 0; o >>= 1) s12[c] += __shfl_xor(s12[c], o);
#pragma unroll
    for (int v = 0; v < kBlkVec; ++v)
#pragma unroll
      for (int o = LG / 2; o > 0; o >>= 1) s3[v] += __shfl_xor(s3[v], o);
    if (l == 0 && j < n) {
      const double qv = q[j];
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v) {
        const f64x2 t = *reinterpret_cast<const f64x2*>(xg + (size_t)j * kBlkCols + 2 * v);  // {g, x}
        const double s1 = s12[2 * v], s2 = s12[2 * v + 1], p2 = -s2;
        if (SQ) tv[(size_t)j * kBlkVec + v] = p2;
        if (v < kt) {
          const double gsv = t.x - s1 - sigma * s2;
          const double dx = eta > 0.0 ? t.y - (XK ? XK[(size_t)v * n + j] : 0.0) : 0.0;
          if (GS) GS[(size_t)v * n + j] = gsv;
          if (GX) GX[(size_t)v * n + j] = gsv + (sigma - qv) * p2 + rho * s3[v] + eta * dx;
          red[2 * v + 1] += dx * dx;
        }
      }
    }
  }
  {
    const int64_t chunk = ((int64_t)m + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < m ? lo + chunk : m;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
      const size_t dst = (size_t)(rperm ? rperm[p] : p);
#pragma unroll
      for (int v = 0; v < kBlkVec; ++v) {
        if (v < kt) {
          const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * kBlkCols + 2 * v);
          const double yv = t.x + sigma * t.y;
          if (YS) YS[(size_t)v * m + dst] = yv;
          red[2 * v] += keep[(size_t)p * kBlkVec + v] * yv;
        }
      }
    }
  }
  bq_block_sum(red, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < kBlkCols; ++c) part[(size_t)blockIdx.x * kBlkCols + c] = red[c];
  }
}

// The scalars of a tile from the workgroups' partials, column by column, each sum in index order as in k_bq_phi (one
// workgroup): out[v] = {phi, f, c.c, c.ys, |x - xk|^2}_v, phi = f - c.ys + rho/2 c.c + eta/2 |x - xk|^2.  f comes from partF
// ([nF][kBlkVec], k_bqb_og_pack_sq) when that is given, else from partP[.][v][0]; partP, partE: [nP], [nE][kBlkVec][2].
__global__ __launch_bounds__(256) void k_bqb_phi(const double* __restrict__ partF, int nF, const double* __restrict__ partP,
                                                 int nP, const double* __restrict__ partE, int nE, double rho, double eta,
                                                 double* __restrict__ out) {
  __shared__ double sh[16];
  const int cf = (nF + 255) / 256, cp = (nP + 255) / 256, ce = (nE + 255) / 256;
  for (int v = 0; v < kBlkVec; ++v) {
    double red[4] = {0.0, 0.0, 0.0, 0.0};
    if (partF)
      for (int i = threadIdx.x * cf; i < min(nF, ((int)threadIdx.x + 1) * cf); ++i) red[0] += partF[(size_t)i * kBlkVec + v];
    for (int i = threadIdx.x * cp; i < min(nP, ((int)threadIdx.x + 1) * cp); ++i) {
      if (!partF) red[0] += partP[(size_t)i * kBlkCols + 2 * v];
      red[1] += partP[(size_t)i * kBlkCols + 2 * v + 1];
    }
    for (int i = threadIdx.x * ce; i < min(nE, ((int)threadIdx.x + 1) * ce); ++i) {
      red[2] += partE[(size_t)i * kBlkCols + 2 * v];
      red[3] += partE[(size_t)i * kBlkCols + 2 * v + 1];
    }
    bq_block_sum(red, sh);
    if (threadIdx.x == 0) {
      double phi = red[0] - red[2];
      phi += 0.5 * rho * red[1];
      phi += 0.5 * eta * red[3];
      out[v * 5] = phi;
      out[v * 5 + 1] = red[0];
      out[v * 5 + 2] = red[1];
      out[v * 5 + 3] = red[2];
      out[v * 5 + 4] = red[3];
    }
  }
}

// ---- bordered band (fpsq_band_create_bordered): the s <= kBorderMax rows of A stored LAST couple with every row of M,
//   M = [B C; C' D],  B = A_b A_b' + delta I (mb x mb, the band the sweeps factor),  C = A_b A_s',  D = A_s A_s' + delta I.
// A factorisation keeps C and Z = B^-1 C as [.][16] arrays (columns >= s zero) and the Cholesky factor of S = D - C'Z; an
// M-solve is the sweeps on the band rows, which leave y = B^-1 r in rows < mb and the border's right-hand side t untouched
// in rows mb .. mb + s - 1 (the sweeps pass over rows >= mb at most as padding rows of the last block: identity pivots, zero
// couplings), followed by k_border_reduce and k_border_update:  w = S^-1 (t - C'y),  u = y - Z w.
// NC = interleaved right-hand-side columns of the sweeps' array (2: k_trsv_chain / k_trsv_step3, 16: k_trsm_chain16).  Every
// sum has a fixed order that depends on the shape alone (rows in index order inside a workgroup's slice, slices and then
// workgroups in index order, the 16 border columns in index order), column c reads column c only: a column's bits depend
// neither on its position, nor on its neighbours, nor on how many there are.  No atomics, no waits.
constexpr int kBorderMax = 16;
constexpr int kBorderGrid = 128;  // most workgroups of the two kernels (every update workgroup re-sums all the partials)

// part[blk][i][c] = sum over this workgroup's band rows p of C[p][i] y[p][c];  workgroup 0 also saves t (tsave[i][c] =
// y[mb + i][c], zero for i >= s), which k_border_update overwrites with w
template <int NC>
__global__ __launch_bounds__(256) void k_border_reduce(const double* __restrict__ Cm, const double* __restrict__ y, int mb,
                                                       int s, double* __restrict__ part, double* __restrict__ tsave) {
  constexpr int NO = kBorderMax * NC;  // sums of a workgroup
  constexpr int NS = 256 / NO;         // row slices: thread = (slice, sum)
  __shared__ double sh[256];
  const int o = threadIdx.x % NO, sl = threadIdx.x / NO, i = o / NC, c = o % NC;
  const int chunk = (mb + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = min(mb, (int)blockIdx.x * chunk), hi = min(mb, lo + chunk);
  double a = 0.0;
  for (int p = lo + sl; p < hi; p += NS) a += Cm[(size_t)p * kBorderMax + i] * y[(size_t)p * NC + c];
  if (NS > 1) {
    sh[threadIdx.x] = a;
    __syncthreads();
    if (sl == 0)
      for (int q = 1; q < NS; ++q) a += sh[q * NO + o];
  }
  if (sl == 0) {
    part[(size_t)blockIdx.x * NO + o] = a;
    if (blockIdx.x == 0) tsave[o] = i < s ? y[(size_t)(mb + i) * NC + c] : 0.0;
  }
}

// every workgroup: g = t - sum of the partials (index order), w = L'^-1 L^-1 g (one thread per column), then its own slice
// of the band rows, y[p][c] -= sum_i Z[p][i] w[i][c]; workgroup 0 writes w into the border rows.  Ls: the factor of S,
// [16][16] row-major, lower, identity beyond s.
template <int NC>
__global__ __launch_bounds__(256) void k_border_update(const double* __restrict__ Zm, const double* __restrict__ Ls,
                                                       const double* __restrict__ part, int nparts,
                                                       const double* __restrict__ tsave, double* y, int mb, int s) {
  constexpr int NO = kBorderMax * NC;
  __shared__ double L[kBorderMax * kBorderMax];
  __shared__ double g[NO];
  L[threadIdx.x] = Ls[threadIdx.x];
  if (threadIdx.x < NO) {
    double a = 0.0;
    for (int q = 0; q < nparts; ++q) a += part[(size_t)q * NO + threadIdx.x];
    g[threadIdx.x] = tsave[threadIdx.x] - a;
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    const int c = threadIdx.x;
    double w[kBorderMax];
#pragma unroll
    for (int i = 0; i < kBorderMax; ++i) {
      double v = g[i * NC + c];
#pragma unroll
      for (int k = 0; k < i; ++k) v -= L[i * kBorderMax + k] * w[k];
      w[i] = v / L[i * kBorderMax + i];
    }
#pragma unroll
    for (int i = kBorderMax - 1; i >= 0; --i) {
      double v = w[i];
#pragma unroll
      for (int k = i + 1; k < kBorderMax; ++k) v -= L[k * kBorderMax + i] * w[k];
      w[i] = v / L[i * kBorderMax + i];
    }
#pragma unroll
    for (int i = 0; i < kBorderMax; ++i) g[i * NC + c] = w[i];
  }
  __syncthreads();
  const int chunk = (mb + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = min(mb, (int)blockIdx.x * chunk), hi = min(mb, lo + chunk);
  for (int64_t idx = (int64_t)lo * NC + threadIdx.x; idx < (int64_t)hi * NC; idx += 256) {
    const int64_t p = idx / NC;
    const int c = (int)(idx % NC);
    const double* z = Zm + (size_t)p * kBorderMax;
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < kBorderMax; ++i) a += z[i] * g[i * NC + c];
    y[idx] -= a;
  }
  if (blockIdx.x == 0 && threadIdx.x < NO && (int)threadIdx.x / NC < s)
    y[(size_t)mb * NC + threadIdx.x] = g[threadIdx.x];  // (row mb + i, column c: i * NC + c behind row mb)
}

// xg[colind[k]][i] = vals[k] over the entries of border row i (stored row mb + i): A_s' as the interleaved [n][16] tile the
// block A product multiplies (the tile is zeroed first; a row holds a column once)
__global__ __launch_bounds__(256) void k_border_scatter(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                        const double* __restrict__ vals, int mb, double* __restrict__ xg) {
  const int i = blockIdx.x;
  for (int k = rowptr[mb + i] + threadIdx.x; k < rowptr[mb + i + 1]; k += 256) xg[(size_t)colind[k] * kBlkCols + i] = vals[k];
}

// One workgroup: S = D + delta I - C'Z from the partials of C'Z (k_border_reduce<16> on Z, summed in index order) and the
// rows mb .. mb + s - 1 of CD = A A_s' (lower triangle), then its Cholesky factor into Ls ([16][16], identity beyond s).
// Pivots by the rule of wave_diag16: one that is not above tol (0 when no regularisation is set) is replaced by reg (1 when
// none is set) and counted in info[1] resp. reported in info[0] as stored row mb + j, 1-based.  info[0] keeps the LOWEST stored
// row, as in wave_diag16: the border rows are stored last and this kernel runs after the band's, so writing only into an empty
// word (and the first j of this kernel) is that rule.
__global__ __launch_bounds__(256) void k_border_chol(const double* __restrict__ part, int nparts, const double* __restrict__ CD,
                                                     int mb, int s, double delta, double tol, double reg,
                                                     double* __restrict__ Ls, int* info) {
  __shared__ double S[kBorderMax][kBorderMax + 1];
  const int i = threadIdx.x / kBorderMax, j = threadIdx.x % kBorderMax;
  {
    double a = 0.0;
    for (int q = 0; q < nparts; ++q) a += part[(size_t)q * 256 + threadIdx.x];
    double v = i == j ? 1.0 : 0.0;
    if (i < s && j < s) v = (CD[(size_t)(mb + i) * kBorderMax + j] + (i == j ? delta : 0.0)) - a;
    S[i][j] = v;
  }
  __syncthreads();
  const bool dyn = reg > 0.0;
  const double thr = dyn ? tol : 0.0, sub = dyn ? reg : 1.0;
  int nbad = 0, first = 0;
  for (int k = 0; k < s; ++k) {
    if (threadIdx.x == 0) {
      double d = S[k][k];
      if (!(d > thr)) {
        first = nbad == 0 ? k + 1 : first;
        ++nbad;
        d = sub;
      }
      S[k][k] = sqrt(d);
    }
    __syncthreads();
    if (j == k && i > k) S[i][k] /= S[k][k];
    __syncthreads();
    if (j > k && i >= j) S[i][j] -= S[i][k] * S[j][k];
    __syncthreads();
  }
  Ls[threadIdx.x] = j <= i ? S[i][j] : 0.0;
  if (threadIdx.x == 0 && nbad) {
    if (dyn)
      atomicAdd(info + 1, nbad);
    else
      atomicCAS(info, 0, mb + first);
  }
}

// ---- long columns (fpsq_band_create_bordered_cols): the s <= kBorderMax columns of A taken out of the band, A = [A_b | U],
//   M = B + U U',  B = A_b A_b' + delta I (the band the sweeps factor),  M^-1 r = y - Z w,  y = B^-1 r,  Z = B^-1 U,
//   S = I + U'Z,  w = S^-1 (U'y).
// A factorisation keeps U and Z as [.][16] arrays in the stored row order (columns >= s zero) and the Cholesky factor of S; an
// M-solve is the sweeps, then k_border_reduce with U in the place of C and no border rows (the partials of U'y), then
// k_cols_update.  VIRTUAL ROWS: the transposed structure the A' kernels walk holds, for long column i, one entry of value 1
// per workgroup g of the reduction, pointing at row mpad + 16 g + i of the vector -- slots behind the padded rows that no
// sweep touches.  For an operand that is not a solution (keep, the x of fpsq_band_jac_mul(trans = 1)) k_border_reduce writes
// its partials straight into those slots (their layout IS part[g][i][c]); for the solutions k_cols_update leaves w in the
// slots of g = 0 and zero in the others, since U'(y - Z w) = w.  The formation by columns skips a long column by its j <= i
// guard (a virtual row lies beyond every row).  Sums in a fixed order, column c reads column c only, no atomics, no waits.

// U[lc_row[t]][i] = vals[lc_ent[t]] over the entries t of long column i (stored row, stored entry); U is zeroed first
__global__ __launch_bounds__(256) void k_cols_scatter(const int32_t* __restrict__ lc_ptr, const int32_t* __restrict__ lc_row,
                                                      const int32_t* __restrict__ lc_ent, const double* __restrict__ vals,
                                                      double* __restrict__ U) {
  const int i = blockIdx.x, e = lc_ptr[i + 1];
  for (int t = lc_ptr[i] + (int)blockIdx.y * 256 + (int)threadIdx.x; t < e; t += (int)gridDim.y * 256)
    U[(size_t)lc_row[t] * kBorderMax + i] = vals[lc_ent[t]];
}

// every workgroup: g = the sum of the partials of U'y (index order), w = L'^-1 L^-1 g (one thread per column), then its own
// slice of the rows, y[p][c] -= sum_i Z[p][i] w[i][c], and its own virtual rows: w for workgroup 0, zero for the others.
// The grid is the grid of the reduction.  Ls: the factor of S, [16][16] row-major, lower, identity beyond s.
template <int NC>
__global__ __launch_bounds__(256) void k_cols_update(const double* __restrict__ Zm, const double* __restrict__ Ls,
                                                     const double* __restrict__ part, int nparts, double* y, int m, int mpad) {
  constexpr int NO = kBorderMax * NC;
  __shared__ double L[kBorderMax * kBorderMax];
  __shared__ double g[NO];
  L[threadIdx.x] = Ls[threadIdx.x];
  if (threadIdx.x < NO) {
    double a = 0.0;
    for (int q = 0; q < nparts; ++q) a += part[(size_t)q * NO + threadIdx.x];
    g[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    const int c = threadIdx.x;
    double w[kBorderMax];
#pragma unroll
    for (int i = 0; i < kBorderMax; ++i) {
      double v = g[i * NC + c];
#pragma unroll
      for (int k = 0; k < i; ++k) v -= L[i * kBorderMax + k] * w[k];
      w[i] = v / L[i * kBorderMax + i];
    }
#pragma unroll
    for (int i = kBorderMax - 1; i >= 0; --i) {
      double v = w[i];
#pragma unroll
      for (int k = i + 1; k < kBorderMax; ++k) v -= L[k * kBorderMax + i] * w[k];
      w[i] = v / L[i * kBorderMax + i];
    }
#pragma unroll
    for (int i = 0; i < kBorderMax; ++i) g[i * NC + c] = w[i];
  }
  __syncthreads();
  const int chunk = (m + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = min(m, (int)blockIdx.x * chunk), hi = min(m, lo + chunk);
  for (int64_t idx = (int64_t)lo * NC + threadIdx.x; idx < (int64_t)hi * NC; idx += 256) {
    const int64_t p = idx / NC;
    const int c = (int)(idx % NC);
    const double* z = Zm + (size_t)p * kBorderMax;
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < kBorderMax; ++i) a += z[i] * g[i * NC + c];
    y[idx] -= a;
  }
  if (threadIdx.x < NO)  // (virtual row mpad + 16 blk + i, column c: blk * NO + i * NC + c behind row mpad)
    y[(size_t)mpad * NC + (size_t)blockIdx.x * NO + threadIdx.x] = blockIdx.x == 0 ? g[threadIdx.x] : 0.0;
}

// One workgroup: S = I + U'Z from the partials of U'Z (k_border_reduce<16> on Z, summed in index order; the lower triangle
// is used), then its Cholesky factor into Ls ([16][16], identity beyond s) and ratio[0] = (largest / smallest pivot of the
// factor)^2.  Pivots by the rule of k_border_chol; a failing one is reported in info[0] as stored row m, 1-based, and only into
// an empty word: S >= I whenever B is positive definite, so B's failing pivot, at a lower stored position, is there already.
__global__ __launch_bounds__(256) void k_cols_chol(const double* __restrict__ part, int nparts, int s, int m, double tol,
                                                   double reg, double* __restrict__ Ls, double* __restrict__ ratio, int* info) {
  __shared__ double S[kBorderMax][kBorderMax + 1];
  const int i = threadIdx.x / kBorderMax, j = threadIdx.x % kBorderMax;
  {
    double a = 0.0;
    for (int q = 0; q < nparts; ++q) a += part[(size_t)q * 256 + threadIdx.x];
    S[i][j] = (i == j ? 1.0 : 0.0) + (i < s && j < s ? a : 0.0);
  }
  __syncthreads();
  const bool dyn = reg > 0.0;
  const double thr = dyn ? tol : 0.0, sub = dyn ? reg : 1.0;
  int nbad = 0;
  for (int k = 0; k < s; ++k) {
    if (threadIdx.x == 0) {
      double d = S[k][k];
      if (!(d > thr)) {
        ++nbad;
        d = sub;
      }
      S[k][k] = sqrt(d);
    }
    __syncthreads();
    if (j == k && i > k) S[i][k] /= S[k][k];
    __syncthreads();
    if (j > k && i >= j) S[i][j] -= S[i][k] * S[j][k];
    __syncthreads();
  }
  Ls[threadIdx.x] = j <= i ? S[i][j] : 0.0;
  if (threadIdx.x == 0) {
    double lo = S[0][0], hi = S[0][0];
    for (int k = 1; k < s; ++k) {
      lo = fmin(lo, S[k][k]);
      hi = fmax(hi, S[k][k]);
    }
    ratio[0] = (hi / lo) * (hi / lo);
    if (nbad) {
      if (dyn)
        atomicAdd(info + 1, nbad);
      else
        atomicCAS(info, 0, m);
    }
  }
}

// ---- arrow band (fpsq_band_create_arrow): border rows AND long columns on one handle.  Stored order: the mb band rows, then
// the s_r border rows; L = the s_c long columns, "o" = the other columns,
//   M = M_r + U U',   U = [U_b; U_s] (all m rows),   M_r = [B C; C' D],  B = A_b,o A_b,o' + delta I,  C = A_b,o A_s,o',
//   D = A_s,o A_s,o' + delta I.
// M_r^-1 is the bordered band's solve (Z_r = B^-1 C, S_r = D - C'Z_r), the long columns' correction is wrapped around it
// (Z_c = M_r^-1 U, S_c = I + U'Z_c).  NESTED form of an M-solve: the sweeps, k_border_reduce / k_border_update, k_border_reduce
// / k_cols_update (four launches).  FUSED form (two launches): with y the sweeps' output and t the border's right-hand side,
//   w_r = S_r^-1 (t - C'y),   U'M_r^-1 r = U_b'y + G w_r,   G = U_s' - U_b'Z_r (s_c x s_r, formed once per factorisation),
//   w_c = S_c^-1 (U_b'y + G w_r),   u = y - Z_r w_r - Z_c,b w_c on the band rows,   w_r - Z_c,s w_c on the border rows,
// so k_arrow_reduce forms the partials of C'y and of U_b'y in ONE pass over y and k_arrow_update corrects every row once.  The
// virtual rows receive w_c as k_cols_update leaves it.  Sums in a fixed order that depends on the shape alone, column c reads
// column c only, no atomics, no waits: the contract of the two corrections above.

// xg[lcols[i]][0 .. 15] = 0: the rows of the border's scattered tile at the long columns, so that the block A product forms
// [C; D - delta I] = A_o A_s,o' although A's rows hold the long columns' entries
__global__ __launch_bounds__(256) void k_arrow_clear(const int32_t* __restrict__ lcols, int s_c, double* __restrict__ xg) {
  const int i = threadIdx.x / kBlkCols, c = threadIdx.x % kBlkCols;
  if (i < s_c) xg[(size_t)lcols[i] * kBlkCols + c] = 0.0;
}

// One workgroup: G[i][j] = U[mb + j][i] - sum of the partials of U_b'Z_r (k_border_reduce<16> with U for C and Z_r for y,
// summed in index order), zero beyond s_c resp. s_r; [16][16] row-major
__global__ __launch_bounds__(256) void k_arrow_g(const double* __restrict__ part, int nparts, const double* __restrict__ U, int mb,
                                                 int s_r, int s_c, double* __restrict__ G) {
  const int i = threadIdx.x / kBorderMax, j = threadIdx.x % kBorderMax;
  double a = 0.0;
  for (int q = 0; q < nparts; ++q) a += part[(size_t)q * 256 + threadIdx.x];
  G[threadIdx.x] = i < s_c && j < s_r ? U[(size_t)(mb + j) * kBorderMax + i] - a : 0.0;
}

// partR[blk][i][c] = sum over this workgroup's band rows p of C[p][i] y[p][c], partC[blk][i][c] the same with U_b; workgroup 0
// also saves t (tsave[i][c] = y[mb + i][c], zero for i >= s).  The slices and their order are k_border_reduce's.
template <int NC>
__global__ __launch_bounds__(256) void k_arrow_reduce(const double* __restrict__ Cm, const double* __restrict__ Um,
                                                      const double* __restrict__ y, int mb, int s, double* __restrict__ partR,
                                                      double* __restrict__ partC, double* __restrict__ tsave) {
  constexpr int NO = kBorderMax * NC;
  constexpr int NS = 256 / NO;
  __shared__ double shr[256], shc[256];
  const int o = threadIdx.x % NO, sl = threadIdx.x / NO, i = o / NC, c = o % NC;
  const int chunk = (mb + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = min(mb, (int)blockIdx.x * chunk), hi = min(mb, lo + chunk);
  double ar = 0.0, ac = 0.0;
  for (int p = lo + sl; p < hi; p += NS) {
    const double v = y[(size_t)p * NC + c];
    ar += Cm[(size_t)p * kBorderMax + i] * v;
    ac += Um[(size_t)p * kBorderMax + i] * v;
  }
  if (NS > 1) {
    shr[threadIdx.x] = ar;
    shc[threadIdx.x] = ac;
    __syncthreads();
    if (sl == 0)
      for (int q = 1; q < NS; ++q) {
        ar += shr[q * NO + o];
        ac += shc[q * NO + o];
      }
  }
  if (sl == 0) {
    partR[(size_t)blockIdx.x * NO + o] = ar;
    partC[(size_t)blockIdx.x * NO + o] = ac;
    if (blockIdx.x == 0) tsave[o] = i < s ? y[(size_t)(mb + i) * NC + c] : 0.0;
  }
}

// g[.][c] <- L'^-1 L^-1 g[.][c] (L: [16][16] row-major, lower, identity beyond its order), the solve of the two update kernels
template <int NC>
__device__ __forceinline__ void arrow_solve16(const double* L, double* g, int c) {
  double w[kBorderMax];
#pragma unroll
  for (int i = 0; i < kBorderMax; ++i) {
    double v = g[i * NC + c];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i * kBorderMax + k] * w[k];
    w[i] = v / L[i * kBorderMax + i];
  }
#pragma unroll
  for (int i = kBorderMax - 1; i >= 0; --i) {
    double v = w[i];
#pragma unroll
    for (int k = i + 1; k < kBorderMax; ++k) v -= L[k * kBorderMax + i] * w[k];
    w[i] = v / L[i * kBorderMax + i];
  }
#pragma unroll
  for (int i = 0; i < kBorderMax; ++i) g[i * NC + c] = w[i];
}

// every workgroup: both sets of partials (nparts of each, the reduction's grid) re-summed in index order, w_r = S_r^-1 (t -
// C'y), w_c = S_c^-1 (U_b'y + G w_r), then its own slice of ALL m rows (the grid is the long columns' grid, over m): band rows
// y -= Z_r w_r + Z_c w_c, border rows y = w_r - Z_c w_c; and its own virtual rows, w_c for workgroup 0, zero for the others.
template <int NC>
__global__ __launch_bounds__(256) void k_arrow_update(const double* __restrict__ Zr, const double* __restrict__ Lrs,
                                                      const double* __restrict__ Zc, const double* __restrict__ Lcs,
                                                      const double* __restrict__ Gm, const double* __restrict__ partR,
                                                      const double* __restrict__ partC, int nparts,
                                                      const double* __restrict__ tsave, double* y, int mb, int m, int mpad) {
  constexpr int NO = kBorderMax * NC;
  __shared__ double Lr[kBorderMax * kBorderMax], Lc[kBorderMax * kBorderMax], G[kBorderMax * kBorderMax];
  __shared__ double gr[NO], gc[NO];
  Lr[threadIdx.x] = Lrs[threadIdx.x];
  Lc[threadIdx.x] = Lcs[threadIdx.x];
  G[threadIdx.x] = Gm[threadIdx.x];
  if (threadIdx.x < NO) {
    double a = 0.0, u = 0.0;
    for (int q = 0; q < nparts; ++q) {
      a += partR[(size_t)q * NO + threadIdx.x];
      u += partC[(size_t)q * NO + threadIdx.x];
    }
    gr[threadIdx.x] = tsave[threadIdx.x] - a;
    gc[threadIdx.x] = u;
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    const int c = threadIdx.x;
    arrow_solve16<NC>(Lr, gr, c);
    for (int i = 0; i < kBorderMax; ++i) {
      double v = gc[i * NC + c];
#pragma unroll
      for (int j = 0; j < kBorderMax; ++j) v += G[i * kBorderMax + j] * gr[j * NC + c];
      gc[i * NC + c] = v;
    }
    arrow_solve16<NC>(Lc, gc, c);
  }
  __syncthreads();
  const int chunk = (m + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = min(m, (int)blockIdx.x * chunk), hi = min(m, lo + chunk);
  for (int64_t idx = (int64_t)lo * NC + threadIdx.x; idx < (int64_t)hi * NC; idx += 256) {
    const int64_t p = idx / NC;
    const int c = (int)(idx % NC);
    const double* zc = Zc + (size_t)p * kBorderMax;
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < kBorderMax; ++i) a += zc[i] * gc[i * NC + c];
    if (p < mb) {
      const double* zr = Zr + (size_t)p * kBorderMax;
      double r = 0.0;
#pragma unroll
      for (int i = 0; i < kBorderMax; ++i) r += zr[i] * gr[i * NC + c];
      y[idx] = (y[idx] - r) - a;
    } else {
      y[idx] = gr[(int)(p - mb) * NC + c] - a;
    }
  }
  if (threadIdx.x < NO)  // (virtual row mpad + 16 blk + i, column c: blk * NO + i * NC + c behind row mpad)
    y[(size_t)mpad * NC + (size_t)blockIdx.x * NO + threadIdx.x] = blockIdx.x == 0 ? gc[threadIdx.x] : 0.0;
}

}  // namespace fpsq
