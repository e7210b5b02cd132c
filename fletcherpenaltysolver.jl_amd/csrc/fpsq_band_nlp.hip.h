// fpsq_band_nlp.hip.h -- part of the fpsq_band.hip translation unit (included behind the fpsq_band_qp_* group): the
// device-resident model with NONLINEAR equality constraints on the banded handle (C ABI: include/fpsq.h, fpsq_band_nlp_*).
//   f(x) = 1/2 x' diag(q) x + d'x,   c_i(x) = sum_j (A_ij + 1/2 H_ij x_j) x_j - b_i,   H on the pattern of A,
// so J(x)_ij = A_ij + H_ij x_j has the handle's pattern for every x, sum_i y_i Hess c_i = diag(H'y) and
// ghjvprod(x, g, v) = H (g .* v): everything nonlinear is a product with the pattern the handle holds and a second value
// array.  The kernels follow k_bq_* (fpsq_band.hip.h): a lane group per row, grid-stride tiles, sums in a fixed order
// (lanes by xor shuffles, waves and workgroups in index order), no floating-point atomics.
#pragma once

namespace fpsq {

// vals[k] = a[k] + h[k] x[colind[k]] over the stored CSR: J(x) where k_band_form_t and the A products read it
__global__ __launch_bounds__(256) void k_bn_vals(const double* __restrict__ a, const double* __restrict__ h,
                                                 const int32_t* __restrict__ colind, const double* __restrict__ x,
                                                 double* __restrict__ vals, int64_t nnz) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256)
    vals[k] = a[k] + h[k] * x[colind[k]];
}

// The same in the transposed CSR, a lane group per row j (a column of J): t_vals[k] = ta[k] + th[k] x[j]; x_j is read once
// per row, nothing is gathered
template <int LG>
__global__ __launch_bounds__(256) void k_bn_tvals(const int32_t* __restrict__ t_rowptr, const double* __restrict__ ta,
                                                  const double* __restrict__ th, const double* __restrict__ x,
                                                  double* __restrict__ t_vals, int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    if (j >= n) continue;
    const double xv = x[j];
    const int e = t_rowptr[j + 1];
    for (int k = t_rowptr[j] + l; k < e; k += LG) t_vals[k] = ta[k] + th[k] * xv;
  }
}

// The prologue of an objgrad: one pass over the stored CSR reading J (vals), h and the packed pair xg[c] = {g_c, x_c}
// (k_bq_pack<false>): c_p = sum (J - 1/2 h x_c) x_c - b_p, r[p] = {(J g)_p, -c_p} where the sweeps read it (zero on the
// padding), keep[p] = c_p; part[2 blk] = this workgroup's slice of f = x.(1/2 q x + d), part[2 blk + 1] = of c.c
template <int LG>
__global__ __launch_bounds__(256) void k_bn_prologue(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                     const double* __restrict__ vals, const double* __restrict__ h,
                                                     const double* __restrict__ xg, const double* __restrict__ x,
                                                     const double* __restrict__ q, const double* __restrict__ d,
                                                     const double* __restrict__ bp, double* __restrict__ r,
                                                     double* __restrict__ keep, double* __restrict__ part, int m, int mpad,
                                                     int n) {
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
        const double jv = vals[k], hv = h[k];
        const f64x2 t = *reinterpret_cast<const f64x2*>(xg + (size_t)colind[k] * 2);
        a0 += jv * t.x;
        a1 += (jv - 0.5 * hv * t.y) * t.y;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) {
      a0 += __shfl_xor(a0, o);
      a1 += __shfl_xor(a1, o);
    }
    if (l == 0 && p < mpad) {  // (a0 = a1 = 0 on the padding rows)
      double cv = 0.0, r1 = 0.0;
      if (p < m) {
        cv = a1 - bp[p];
        r1 = -cv;
        red[1] += cv * cv;
      }
      *reinterpret_cast<f64x2*>(r + (size_t)p * 2) = f64x2{a0, r1};
      keep[p] = cv;
    }
  }
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

// c(x) alone, from the model's own arrays (no factorisation has to have put J into the handle), in the caller's row order
// (rperm: stored row -> the caller's, null = identity): c_p = sum (a + 1/2 h x_c) x_c - b_p
template <int LG>
__global__ __launch_bounds__(256) void k_bn_cons(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                 const double* __restrict__ a, const double* __restrict__ h,
                                                 const double* __restrict__ x, const double* __restrict__ bp,
                                                 const int32_t* __restrict__ rperm, double* __restrict__ c, int m) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (m + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * RPB + g;
    double s = 0.0;
    if (p < m) {
      const int e = rowptr[p + 1];
      for (int k = rowptr[p] + l; k < e; k += LG) {
        const double xv = x[colind[k]];
        s += (a[k] + 0.5 * h[k] * xv) * xv;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && p < m) c[rperm ? rperm[p] : p] = s - bp[p];
  }
}

// The epilogue of an objgrad: one pass over the transposed CSR reading TWO value arrays (J' = t_vals, H' = th) against three
// m-vectors (y[p] = {q1, q2}, keep = c), six sums per row j: s1 = (J'q1)_j, s2 = (J'q2)_j, s3 = (J'c)_j, h1 = (H'q1)_j,
// h2 = (H'q2)_j, h3 = (H'c)_j.  With g_j = q_j x_j + d_j:
//   gs_j = g_j - s1 - sigma s2,  p2_j = -s2,  qe_j = q_j - (h1 + sigma h2) = (q - H'ys)_j,  hc_j = h3,
//   gx_j = gs_j - qe_j p2_j + sigma p2_j + h2 gs_j + rho s3 + eta (x_j - xk_j)       (the gradient in the -ys form)
// qe, hc, gsm (the model's own copies, what fpsq_band_nlp_hprod runs on) are always written; out, gs, ys, xk may be null.
// ys and the partials part[2 blk] = slice of c.ys, part[2 blk + 1] = of |x - xk|^2 as in k_bq_epilogue.
template <int LG>
__global__ __launch_bounds__(256) void k_bn_epilogue(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                     const double* __restrict__ t_vals, const double* __restrict__ th,
                                                     const double* __restrict__ y, const double* __restrict__ keep,
                                                     const int32_t* __restrict__ rperm, const double* __restrict__ x,
                                                     const double* __restrict__ xk, const double* __restrict__ q,
                                                     const double* __restrict__ d, double sigma, double rho, double eta,
                                                     double* __restrict__ out, double* __restrict__ gs, double* __restrict__ ys,
                                                     double* __restrict__ qe, double* __restrict__ hc, double* __restrict__ gsm,
                                                     double* __restrict__ part, int n, int m) {
  constexpr int RPB = 256 / LG;
  __shared__ double sh[8];
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  double red[2] = {0.0, 0.0};
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0;
    if (j < n) {
      const int e = t_rowptr[j + 1];
      for (int k = t_rowptr[j] + l; k < e; k += LG) {
        const double jv = t_vals[k], hv = th[k];
        const int p = t_colind[k];
        const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
        const double cv = keep[p];
        s1 += jv * t.x;
        s2 += jv * t.y;
        s3 += jv * cv;
        h1 += hv * t.x;
        h2 += hv * t.y;
        h3 += hv * cv;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
      s3 += __shfl_xor(s3, o);
      h1 += __shfl_xor(h1, o);
      h2 += __shfl_xor(h2, o);
      h3 += __shfl_xor(h3, o);
    }
    if (l == 0 && j < n) {
      const double xv = x[j], qv = q[j];
      const double gsv = (qv * xv + d[j]) - s1 - sigma * s2, p2 = -s2;
      const double qev = qv - (h1 + sigma * h2);
      const double dx = eta > 0.0 ? xv - (xk ? xk[j] : 0.0) : 0.0;
      qe[j] = qev;
      hc[j] = h3;
      gsm[j] = gsv;
      if (gs) gs[j] = gsv;
      if (out) out[j] = gsv + (sigma - qev) * p2 + h2 * gsv + rho * s3 + eta * dx;
      red[1] += dx * dx;
    }
  }
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

// hprod Val(2), behind the unchanged k_bq_epilogue<LG, true> (q = qe): Hv += hc .* v   (:560-562: Hcv is not scaled by rho)
__global__ __launch_bounds__(256) void k_bn_hcv(const double* __restrict__ hc, const double* __restrict__ v,
                                                double* __restrict__ Hv, int n) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) Hv[j] += hc[j] * v[j];
}

// The epilogue of an hprod Val(1) (:572-634): the hprod rows of k_bq_epilogue with q = qe -- y[p] = {q1, q2} the solutions
// for {J v, J (qe v)}, keep = J v; s1 = (J'q1)_j = Ptv_j, s2 = (J'q2)_j, s3 = (J'J v)_j -- and a fourth sum h1 = (H'q1)_j:
//   Hv_j = (qe_j v_j - s2) - qe_j s1 + 2 sigma s1 + rho (s3 + hc_j v_j) + eta v_j - h1 gs_j        (:612-614, :626)
template <int LG>
__global__ __launch_bounds__(256) void k_bn_epilogue_h1(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                        const double* __restrict__ t_vals, const double* __restrict__ th,
                                                        const double* __restrict__ y, const double* __restrict__ keep,
                                                        const double* __restrict__ v, const double* __restrict__ qe,
                                                        const double* __restrict__ hc, const double* __restrict__ gsm,
                                                        double sigma, double rho, double eta, double* __restrict__ out, int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, h1 = 0.0;
    if (j < n) {
      const int e = t_rowptr[j + 1];
      for (int k = t_rowptr[j] + l; k < e; k += LG) {
        const double jv = t_vals[k];
        const int p = t_colind[k];
        const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
        s1 += jv * t.x;
        s2 += jv * t.y;
        s3 += jv * keep[p];
        h1 += th[k] * t.x;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
      s3 += __shfl_xor(s3, o);
      h1 += __shfl_xor(h1, o);
    }
    if (l == 0 && j < n) {
      const double vv = v[j], qv = qe[j];
      out[j] = (qv * vv - s2) - qv * s1 + 2.0 * sigma * s1 + rho * (s3 + hc[j] * vv) + eta * vv - h1 * gsm[j];
    }
  }
}

// Ssv = ghjvprod(x, gs, v) = H (gs .* v) (:600) over the stored CSR, straight into the sweeps' right-hand-side layout:
// r[p] = {Ssv_p, 0}, zero on the padding
template <int LG>
__global__ __launch_bounds__(256) void k_bn_hgv(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                const double* __restrict__ h, const double* __restrict__ gsm,
                                                const double* __restrict__ v, double* __restrict__ r, int m, int mpad) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (mpad + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * RPB + g;
    double s = 0.0;
    if (p < m) {
      const int e = rowptr[p + 1];
      for (int k = rowptr[p] + l; k < e; k += LG) {
        const int c = colind[k];
        s += h[k] * (gsm[c] * v[c]);
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && p < mpad) *reinterpret_cast<f64x2*>(r + (size_t)p * 2) = f64x2{s, 0.0};
  }
}

// out_j -= (J'z)_j with z = column 0 of the sweeps' solution y[p] = {z_p, .}   (:606, :612)
template <int LG>
__global__ __launch_bounds__(256) void k_bn_jtz(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                const double* __restrict__ t_vals, const double* __restrict__ y,
                                                double* __restrict__ out, int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s = 0.0;
    if (j < n) {
      const int e = t_rowptr[j + 1];
      for (int k = t_rowptr[j] + l; k < e; k += LG) s += t_vals[k] * y[(size_t)t_colind[k] * 2];
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && j < n) out[j] -= s;
  }
}

// ---- long columns (fpsq_band_nlp_create_arrow).  In the transposed structure long column i (column j = lcols[i]) has no real
// entries: its vgrid virtual entries gather the value 1 (ta = 1, th = 0) and point at the virtual rows mpad + 16 g + i, where
// the solutions hold w (g = 0, zero elsewhere) and `keep` the chunk sums of U'keep.  The J' sums of the kernels above are
// therefore complete at j; the H' sums come out 0.  These two kernels form them from h over the column's own entries, ONE
// WORKGROUP PER LONG COLUMN behind the epilogue, and write that row's outputs again.  Sums in a fixed order (a thread's entries
// in index order, lanes by xor shuffles, waves in index order), no atomics.

// six sums of long column i over the workgroup, in thread 0: v[0 .. 2] = (J'q1)_j, (J'q2)_j, (J'keep)_j from the virtual rows,
// v[3 .. 5] = (H'q1)_j, (H'q2)_j, (H'keep)_j from h
__device__ __forceinline__ void bn_lc_sums(const int32_t* __restrict__ lc_ptr, const int32_t* __restrict__ lc_row,
                                           const int32_t* __restrict__ lc_ent, const double* __restrict__ h,
                                           const double* __restrict__ y, const double* __restrict__ keep, int mpad, int vgrid,
                                           double (&v)[6], double* sh) {
  const int i = blockIdx.x;
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = 0.0;
  for (int g = threadIdx.x; g < vgrid; g += 256) {
    const size_t row = (size_t)mpad + (size_t)kBorderMax * g + i;
    const f64x2 t = *reinterpret_cast<const f64x2*>(y + row * 2);
    v[0] += t.x;
    v[1] += t.y;
    v[2] += keep[row];
  }
  const int e = lc_ptr[i + 1];
  int k = lc_ptr[i] + threadIdx.x;
  // four entries of a thread per trip: their (dependent, gathered) loads are in flight together; the terms enter the sums in
  // the order of the one-entry loop behind it
  for (; k + 3 * 256 < e; k += 4 * 256) {
    double hv[4], kv[4];
    f64x2 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = lc_row[k + u * 256];
      hv[u] = h[lc_ent[k + u * 256]];
      t[u] = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
      kv[u] = keep[p];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[3] += hv[u] * t[u].x;
      v[4] += hv[u] * t[u].y;
      v[5] += hv[u] * kv[u];
    }
  }
  for (; k < e; k += 256) {
    const double hv = h[lc_ent[k]];
    const int p = lc_row[k];
    const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
    v[3] += hv * t.x;
    v[4] += hv * t.y;
    v[5] += hv * keep[p];
  }
  bq_block_sum(v, sh);
}

// objgrad, behind k_bn_epilogue (which left qe_j = q_j, hc_j = 0 and gx_j without the curvature terms at a long column; gs_j
// and gsm_j hold no H' sum and stay): qe_j, hc_j and gx_j by k_bn_epilogue's formulas with the sums above
__global__ __launch_bounds__(256) void k_bn_lc_epilogue(const int32_t* __restrict__ lc_ptr, const int32_t* __restrict__ lc_row,
                                                        const int32_t* __restrict__ lc_ent, const int32_t* __restrict__ lcols,
                                                        const double* __restrict__ h, const double* __restrict__ y,
                                                        const double* __restrict__ keep, const double* __restrict__ x,
                                                        const double* __restrict__ xk, const double* __restrict__ q,
                                                        const double* __restrict__ gsm, double sigma, double rho, double eta,
                                                        double* __restrict__ out, double* __restrict__ qe,
                                                        double* __restrict__ hc, int mpad, int vgrid) {
  __shared__ double sh[24];
  double v[6];
  bn_lc_sums(lc_ptr, lc_row, lc_ent, h, y, keep, mpad, vgrid, v, sh);
  if (threadIdx.x == 0) {
    const int j = lcols[blockIdx.x];
    const double gsv = gsm[j], p2 = -v[1];
    const double qev = q[j] - (v[3] + sigma * v[4]);
    const double dx = eta > 0.0 ? x[j] - (xk ? xk[j] : 0.0) : 0.0;
    qe[j] = qev;
    hc[j] = v[5];
    if (out) out[j] = gsv + (sigma - qev) * p2 + v[4] * gsv + rho * v[2] + eta * dx;
  }
}

// hprod Val(1), behind k_bn_epilogue_h1 (whose h1 is 0 at a long column): Hv_j by its formula with the sums above
__global__ __launch_bounds__(256) void k_bn_lc_epilogue_h1(const int32_t* __restrict__ lc_ptr, const int32_t* __restrict__ lc_row,
                                                           const int32_t* __restrict__ lc_ent, const int32_t* __restrict__ lcols,
                                                           const double* __restrict__ h, const double* __restrict__ y,
                                                           const double* __restrict__ keep, const double* __restrict__ vec,
                                                           const double* __restrict__ qe, const double* __restrict__ hc,
                                                           const double* __restrict__ gsm, double sigma, double rho, double eta,
                                                           double* __restrict__ out, int mpad, int vgrid) {
  __shared__ double sh[24];
  double v[6];
  bn_lc_sums(lc_ptr, lc_row, lc_ent, h, y, keep, mpad, vgrid, v, sh);
  if (threadIdx.x == 0) {
    const int j = lcols[blockIdx.x];
    const double vv = vec[j], qv = qe[j];
    out[j] = (qv * vv - v[1]) - qv * v[0] + 2.0 * sigma * v[0] + rho * (v[2] + hc[j] * vv) + eta * vv - v[3] * gsm[j];
  }
}

}  // namespace fpsq

// ---- host side

// What a model with coupling terms (fpsq_band_nlp_create_coupled, fpsq_band_cnlp.hip.h) holds besides fpsq_band_nlp_s' own arrays:
// the lists of fpsq_coupled.h on the device -- partner lists of the stored and of the transposed entries, the latter's own
// columns, the contributor lists of S -- and the values of Wo(q2), Wo(c) on S.  S itself, -Wo(ys) and the n-vector tv (p2 resp.
// Ptv) are the `lin` view's r_rowptr / r_colind / r_vals / tv.  The buffers are on the model's list.
struct fpsq_band_cnlp_s {
  int32_t *pptr = nullptr, *pcol = nullptr, *tpptr = nullptr, *tpcol = nullptr, *tcol = nullptr;
  double *pw = nullptr, *tpw = nullptr;
  int32_t *cptr = nullptr, *crow = nullptr;
  double *cw = nullptr, *wq2 = nullptr, *wc = nullptr;
  int64_t snz = 0;
};

// fpsq_band_nlp_create: the model's vectors and its two value arrays in the stored row order (a, h: through vperm) and in the
// transposed order (ta, th: through t_perm), gathered once; the three n-vectors an objgrad leaves for the Hessian products;
// `lin`: the view fpsq_band_qp's unchanged kernels take for hprod Val(2) (q = qe).  It borrows the handle's buffers as
// fpsq_band_qp_s does.
struct fpsq_band_nlp_s {
  fpsq_band b = nullptr;
  fpsq_band_cnlp_s* cp = nullptr;  // non-null: the model has coupling terms and runs fpsq_band_cnlp.hip.h's launches
  double *q = nullptr, *d = nullptr, *bp = nullptr;  // n, n, m (b in the STORED row order)
  double *a = nullptr, *h = nullptr, *ta = nullptr, *th = nullptr;  // nnz (+ the virtual entries' slot), t_nnz
  double *qe = nullptr, *hc = nullptr, *gs = nullptr;               // q - H'ys, H'c, gs of the last successful objgrad
  double *partP = nullptr, *partE = nullptr;
  fpsq_band_qp_s lin;
  uint64_t fact_gen = 0;   // the handle's factorisation count when that objgrad ended
  bool evaluated = false;  // an objgrad has succeeded
  std::vector<void*> allocs;
};

extern "C" {

int fpsq_band_nlp_destroy(fpsq_band_nlp nlp) {
  if (!nlp) return FPSQ_ERR_ARG;
  for (void* p : nlp->allocs) hipFree(p);
  delete nlp->cp;
  delete nlp;
  return FPSQ_OK;
}

}  // extern "C"

namespace {
const char kNlpCooRefused[] =
    "the handle was created by a fpsq_band_create_coo entry (its callers do not know the slot order)";

// What the two create entries share, behind their checks of the handle's kind.  With long columns the transposed arrays span
// t_nnz entries and gather a slot behind the stored values (a = 1, h = 0) into the virtual ones; without them t_nnz = nnz and
// every size, lane group and launch is what it was before the handle's kind was looked at.
int band_nlp_make(fpsq_band b, const double* qdiag, const double* d, const double* bvec, const double* a_vals,
                  const double* h_vals, fpsq_band_nlp* out) {
  hipSetDevice(b->device);
  if (!b->scal) {  // the scalars of a call: device side and pinned host side
    if (dalloc(b, &b->scal, 8)) return FPSQ_ERR_HIP;
    CHK(b, hipHostMalloc((void**)&b->scal_host, 64, hipHostMallocDefault));
  }
  if (int rc = wait_input(b)) return rc;  // (device-resident values produced on the registered stream)
  std::vector<double> bh((size_t)b->m), bs((size_t)b->m);
  CHK(b, hipMemcpy(bh.data(), bvec, (size_t)b->m * 8, hipMemcpyDefault));
  for (int64_t p = 0; p < b->m; ++p) bs[p] = bh[b->reordered ? b->rperm_host[p] : p];
  fpsq_band_nlp nlp = new fpsq_band_nlp_s();
  nlp->b = b;
  fpsq_band_qp_s& lin = nlp->lin;
  lin.b = b;
  lin.lgA = lane_group(b->nnz, b->m);
  lin.lgT = lane_group(b->t_nnz, b->n);
  lin.gridP = bq_grid(b->mpad, lin.lgA);
  lin.gridE = bq_grid(b->n, lin.lgT);
  const size_t nb8 = (size_t)b->n * 8, mb8 = (size_t)b->m * 8;
  const size_t zb8 = (size_t)(std::max<int64_t>(b->nnz, 1) + (b->cols ? 1 : 0)) * 8, tb8 = (size_t)std::max<int64_t>(b->t_nnz, 1) * 8;
  if (!qp_buffers(nlp, {{(void**)&nlp->q, nb8, qdiag, hipMemcpyDefault},
                        {(void**)&nlp->d, nb8, d, hipMemcpyDefault},
                        {(void**)&nlp->bp, mb8, bs.data(), hipMemcpyHostToDevice},
                        {(void**)&nlp->a, zb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->h, zb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->ta, tb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->th, tb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->qe, nb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->hc, nb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->gs, nb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->partP, (size_t)lin.gridP * 16, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->partE, (size_t)lin.gridE * 16, nullptr, hipMemcpyDefault}})) {
    b->err = "band_nlp_create: cannot allocate or fill the model's vectors";
    fpsq_band_nlp_destroy(nlp);
    return FPSQ_ERR_HIP;
  }
  lin.q = nlp->qe;
  lin.d = nlp->d;
  lin.bp = nlp->bp;
  lin.partP = nlp->partP;
  lin.partE = nlp->partE;
  // the two value arrays into both orders, by the gathers a factorisation uses for its values
  hipStream_t s = b->stream;
  const dim3 gz((unsigned)std::min<int64_t>((b->nnz + 255) / 256, 4096));
  const dim3 gt((unsigned)std::min<int64_t>((b->t_nnz + 255) / 256, 4096));
  for (int w = 0; w < 2 && b->nnz > 0; ++w) {
    const double* src = w ? h_vals : a_vals;
    double *st = w ? nlp->h : nlp->a, *tr = w ? nlp->th : nlp->ta;
    hipError_t e;
    if (b->cols) {  // the slot the virtual entries gather (nothing is in flight on the array yet)
      const double slot = w ? 0.0 : 1.0;
      if (hipMemcpy(st + b->nnz, &slot, 8, hipMemcpyHostToDevice) != hipSuccess) {
        b->err = "band_nlp_create: cannot read the constraint values";
        fpsq_band_nlp_destroy(nlp);
        return FPSQ_ERR_HIP;
      }
    }
    if (b->reordered) {
      e = hipMemcpyAsync(b->vals_in, src, (size_t)b->nnz * 8, hipMemcpyDefault, s);
      hipLaunchKernelGGL(k_gather_d, gz, dim3(256), 0, s, b->vals_in, b->vperm, st, b->nnz);
    } else {
      e = hipMemcpyAsync(st, src, (size_t)b->nnz * 8, hipMemcpyDefault, s);
    }
    hipLaunchKernelGGL(k_gather_d, gt, dim3(256), 0, s, st, b->t_perm, tr, b->t_nnz);
    if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
      b->err = "band_nlp_create: cannot read the constraint values";
      fpsq_band_nlp_destroy(nlp);
      return FPSQ_ERR_HIP;
    }
  }
  *out = nlp;
  return FPSQ_OK;
}

// a model with coupling terms (nlp->cp): fpsq_band_cnlp.hip.h
int band_cnlp_cons(fpsq_band b, fpsq_band_nlp nlp, const double* x, double* c);
int band_cnlp_objgrad(fpsq_band b, fpsq_band_nlp nlp, const double* x, double sigma, double rho, double eta, double delta,
                      const double* xk, double* fx, double* gx, double* ys, double* gs, int32_t* info);
void band_cnlp_hprod_launches(fpsq_band b, fpsq_band_nlp nlp, const double* v, double sigma, double rho, double eta,
                              int32_t hessian_approx, double* Hv);
}  // namespace

extern "C" {

int fpsq_band_nlp_create(fpsq_band b, const double* qdiag, const double* d, const double* bvec, const double* a_vals,
                         const double* h_vals, fpsq_band_nlp* out) {
  if (!b || !qdiag || !d || !bvec || !out || (b->nnz > 0 && (!a_vals || !h_vals))) return FPSQ_ERR_ARG;
  const char* why = b->border > 0    ? "the handle has border rows"
                    : b->cols > 0    ? "the handle has long columns (they change the transposed structure)"
                    : b->coo_nnz >= 0 ? kNlpCooRefused
                                      : nullptr;
  if (why) {
    b->err = std::string("band_nlp_create: ") + why;
    return FPSQ_ERR_STATE;
  }
  return band_nlp_make(b, qdiag, d, bvec, a_vals, h_vals, out);
}

int fpsq_band_nlp_create_arrow(fpsq_band b, const double* qdiag, const double* d, const double* bvec, const double* a_vals,
                               const double* h_vals, fpsq_band_nlp* out) {
  if (!b || !qdiag || !d || !bvec || !out || (b->nnz > 0 && (!a_vals || !h_vals))) return FPSQ_ERR_ARG;
  if (b->coo_nnz >= 0) {
    b->err = std::string("band_nlp_create_arrow: ") + kNlpCooRefused;
    return FPSQ_ERR_STATE;
  }
  return band_nlp_make(b, qdiag, d, bvec, a_vals, h_vals, out);
}

int fpsq_band_nlp_cons(fpsq_band b, fpsq_band_nlp nlp, const double* x, double* c) {
  if (!b || !nlp || nlp->b != b || !x || !c) return FPSQ_ERR_ARG;
  if (nlp->cp) return band_cnlp_cons(b, nlp, x, c);
  hipSetDevice(b->device);
  if (int rc = wait_input(b)) return rc;
  const StagedArg ax = staged(b, x, b->in_a, (size_t)b->n);
  if (int rc = stage_in(b, ax)) return rc;
  const StagedArg oc = staged(b, c, b->o_q1, (size_t)b->m);
  const int lg = nlp->lin.lgA;
  WITH_LANE_GROUP(lg, hipLaunchKernelGGL(k_bn_cons<LG>, dim3(bq_grid(b->m, lg)), dim3(256), 0, b->stream, b->rowptr, b->colind,
                                         nlp->a, nlp->h, ax.tile(), nlp->bp, b->row_perm(), oc.tile(), (int)b->m))
  if (int rc = stage_back(b, oc)) return rc;
  CHK(b, hipStreamSynchronize(b->stream));
  return FPSQ_OK;
}

int fpsq_band_nlp_objgrad(fpsq_band b, fpsq_band_nlp nlp, const double* x, double sigma, double rho, double eta, double delta,
                          const double* xk, double* fx, double* gx, double* ys, double* gs, int32_t* info) {
  if (!b || !nlp || nlp->b != b || !x || !fx || !(delta >= 0.0)) return FPSQ_ERR_ARG;
  if (nlp->cp) return band_cnlp_objgrad(b, nlp, x, sigma, rho, eta, delta, xk, fx, gx, ys, gs, info);
  hipSetDevice(b->device);
  hipStream_t s = b->stream;
  const fpsq_band_qp_s& lin = nlp->lin;
  const int n = (int)b->n, m = (int)b->m, mpad = (int)b->mpad;
  nlp->evaluated = false;
  b->factored = false;
  if (int rc = wait_input(b)) return rc;
  rho = rho > 0.0 ? rho : 0.0;  // (the reference adds these terms only when the parameter is positive)
  eta = eta > 0.0 ? eta : 0.0;
  const StagedArg ax = staged(b, x, b->in_a, (size_t)n);
  if (int rc = stage_in(b, ax)) return rc;
  const StagedArg axk = staged(b, eta > 0.0 ? xk : nullptr, b->in_b, (size_t)n);
  if (int rc = stage_in(b, axk)) return rc;
  // 1: J(x) into the handle's value arrays, the stored CSR and the transposed one
  b->have_vals = true;
  if (b->nnz > 0) {
    hipLaunchKernelGGL(k_bn_vals, dim3((unsigned)std::min<int64_t>((b->nnz + 255) / 256, 4096)), dim3(256), 0, s, nlp->a, nlp->h,
                       b->colind, ax.tile(), b->vals, b->nnz);
    WITH_LANE_GROUP(lin.lgT, hipLaunchKernelGGL(k_bn_tvals<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, nlp->ta, nlp->th,
                                                ax.tile(), b->t_vals, n))
    if (b->fb_nnz > 0)  // (long columns and k_band_form: the values of the other columns alone, as fpsq_band_factorize)
      hipLaunchKernelGGL(k_gather_d, dim3((unsigned)std::min<int64_t>((b->fb_nnz + 255) / 256, 4096)), dim3(256), 0, s, b->vals,
                         b->fb_perm, b->fb_vals, b->fb_nnz);
  }
  // 2: the numeric factorisation on them
  if (int rc = band_factor_numeric(b, delta, info)) return rc;  // (1: no valid factor, *info says where; nothing is evaluated)
  // 3 - 5: the evaluation on that factor
  if (int rc = eval_begin(b)) return rc;
  const StagedArg ogx = staged(b, gx, b->o_p1, (size_t)n), ogs = staged(b, gs, b->o_p2, (size_t)n),
                  oys = staged(b, ys, b->o_q1, (size_t)m);
  double* keep = b->cols ? b->bd_keep : b->o_q2;  // (long columns: the operand has virtual rows, as in bq_launches)
  hipLaunchKernelGGL(k_bq_pack<false>, grid256(n), dim3(256), 0, s, ax.tile(), nlp->q, nlp->d, b->xn, n);
  WITH_LANE_GROUP(lin.lgA, hipLaunchKernelGGL(k_bn_prologue<LG>, dim3(lin.gridP), dim3(256), 0, s, b->rowptr, b->colind, b->vals,
                                              nlp->h, b->xn, ax.tile(), nlp->q, nlp->d, nlp->bp, b->r2, keep, nlp->partP, m, mpad,
                                              n))
  if (b->cols) cols_keep<1>(b, keep);
  band_solve(b);
  WITH_LANE_GROUP(lin.lgT, hipLaunchKernelGGL(k_bn_epilogue<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind,
                                              b->t_vals, nlp->th, b->r2, keep, b->row_perm(), ax.tile(), axk.tile(), nlp->q, nlp->d,
                                              sigma, rho, eta, ogx.tile(), ogs.tile(), oys.tile(), nlp->qe, nlp->hc, nlp->gs,
                                              nlp->partE, n, m))
  if (b->cols)  // the curvature sums at the long columns, whose transposed rows are virtual
    hipLaunchKernelGGL(k_bn_lc_epilogue, dim3(b->cols), dim3(256), 0, s, b->lc_ptr, b->lc_row, b->lc_ent, b->lc_cols, nlp->h,
                       b->r2, keep, ax.tile(), axk.tile(), nlp->q, nlp->gs, sigma, rho, eta, ogx.tile(), nlp->qe, nlp->hc, mpad,
                       b->bc_grid);
  hipLaunchKernelGGL(k_bq_phi, dim3(1), dim3(256), 0, s, nlp->partP, lin.gridP, nlp->partE, lin.gridE, rho, eta, b->scal);
  for (const StagedArg* o : {&ogx, &ogs, &oys})
    if (int rc = stage_back(b, *o)) return rc;
  if (int rc = eval_end(b, 5, &b->info.last_solve_ms)) return rc;
  *fx = b->scal_host[0];
  nlp->fact_gen = b->fact_gen;
  nlp->evaluated = true;
  return FPSQ_OK;
}

int fpsq_band_nlp_hprod(fpsq_band b, fpsq_band_nlp nlp, const double* v, double sigma, double rho, double eta,
                        int32_t hessian_approx, double* Hv) {
  if (!b || !nlp || nlp->b != b || !v || !Hv) return FPSQ_ERR_ARG;
  if (hessian_approx != 1 && hessian_approx != 2) {
    b->err = "band_nlp_hprod: hessian_approx must be 1 or 2";
    return FPSQ_ERR_ARG;
  }
  if (!nlp->evaluated) {
    b->err = "band_nlp_hprod: no successful fpsq_band_nlp_objgrad of this model yet (it fixes the point of the product)";
    return FPSQ_ERR_STATE;
  }
  if (nlp->fact_gen != b->fact_gen) {
    b->err = "band_nlp_hprod: the handle was factorised again since this model's last objgrad (its values are no longer J(x))";
    return FPSQ_ERR_STATE;
  }
  if (int rc = eval_begin(b)) return rc;
  hipStream_t s = b->stream;
  fpsq_band_qp_s& lin = nlp->lin;
  const int n = (int)b->n, m = (int)b->m, mpad = (int)b->mpad;
  rho = rho > 0.0 ? rho : 0.0;
  eta = eta > 0.0 ? eta : 0.0;
  const StagedArg av = staged(b, v, b->in_a, (size_t)n);
  if (int rc = stage_in(b, av)) return rc;
  const StagedArg ah = staged(b, Hv, b->o_p1, (size_t)n);
  if (nlp->cp) {
    band_cnlp_hprod_launches(b, nlp, av.tile(), sigma, rho, eta, hessian_approx, ah.tile());
  } else if (hessian_approx == 2) {  // the linear model's launches with q = qe, then the curvature of rho/2 |c|^2
    bq_launches(b, &lin, true, av.tile(), nullptr, sigma, rho, eta, ah.tile(), nullptr, nullptr);
    if (rho > 0.0) hipLaunchKernelGGL(k_bn_hcv, grid256(n), dim3(256), 0, s, nlp->hc, av.tile(), ah.tile(), n);
  } else {
    double* keep = b->cols ? b->bd_keep : b->o_q2;
    hipLaunchKernelGGL(k_bq_pack<true>, grid256(n), dim3(256), 0, s, av.tile(), nlp->qe, nlp->d, b->xn, n);
    WITH_LANE_GROUP(lin.lgA, hipLaunchKernelGGL((k_bq_prologue<LG, true, false>), dim3(lin.gridP), dim3(256), 0, s, b->rowptr,
                                                b->colind, b->vals, b->xn, av.tile(), nlp->qe, nlp->d, nlp->bp, b->r2, keep,
                                                nlp->partP, m, mpad, n))
    if (b->cols) cols_keep<1>(b, keep);
    band_solve(b);
    WITH_LANE_GROUP(lin.lgT, hipLaunchKernelGGL(k_bn_epilogue_h1<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind,
                                                b->t_vals, nlp->th, b->r2, keep, av.tile(), nlp->qe, nlp->hc, nlp->gs, sigma, rho,
                                                eta, ah.tile(), n))
    if (b->cols)  // (H'q1)_j at the long columns, before the second solve takes b->r2
      hipLaunchKernelGGL(k_bn_lc_epilogue_h1, dim3(b->cols), dim3(256), 0, s, b->lc_ptr, b->lc_row, b->lc_ent, b->lc_cols, nlp->h,
                         b->r2, keep, av.tile(), nlp->qe, nlp->hc, nlp->gs, sigma, rho, eta, ah.tile(), mpad, b->bc_grid);
    // z = M^-1 H (gs .* v) on the cached factor (tau = delta, include/fpsq.h), Hv -= J'z
    WITH_LANE_GROUP(lin.lgA, hipLaunchKernelGGL(k_bn_hgv<LG>, dim3(lin.gridP), dim3(256), 0, s, b->rowptr, b->colind, nlp->h,
                                                nlp->gs, av.tile(), b->r2, m, mpad))
    band_solve(b);
    WITH_LANE_GROUP(lin.lgT, hipLaunchKernelGGL(k_bn_jtz<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind,
                                                b->t_vals, b->r2, ah.tile(), n))
  }
  if (int rc = stage_back(b, ah)) return rc;
  return eval_end(b, 0, &b->info.last_solve_ms);
}
}  // extern "C"
