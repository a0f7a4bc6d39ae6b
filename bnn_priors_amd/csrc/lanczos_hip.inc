// Effective dimensionality (include/sgmcmc_hip.h, "Lanczos"): one Lanczos step with full reorthogonalisation (two passes of
// classical Gram-Schmidt against every stored row), the symmetric tridiagonal eigensolver (implicit QL, Wilkinson shifts),
// the Ritz vectors U = V^T Y on the fp64 matrix pipe, and N_eff = sum lambda / (lambda + alpha).  Included from
// sgmcmc_hip.hip after numerics_hip.inc (it uses num::qnan, num::is_finite, num::comp_add).
//
// The step kernels are bandwidth-bound GEMVs on vector FMAs: V [rows][D] is read once per pass through its row stride,
// coordinates are cut into chunks of kChunk (one coordinate per thread), workgroup `split` walks the chunks split, split +
// splits, ... and every thread accumulates its coordinate of them in that order; a workgroup's threads are then added by the
// fixed tree of wave_sum / block_sum below and sgmcmc_lanczos_reduce adds the workgroups' partials from 0 upwards.  Nothing
// depends on the row stride or on how many rows there are, and there are no floating-point atomics.
// The Ritz GEMM uses the lane map of v_mfma_f64_16x16x4_f64 that gram_hip.inc's header sets out.

namespace lanczos {

constexpr int kThreads = 256;
constexpr int kChunk = SGMCMC_LANCZOS_CHUNK;            // coordinates of a chunk: one per thread
constexpr int kRows = SGMCMC_LANCZOS_ROWS;              // rows of V per workgroup of the dots pass
constexpr int kMaxM = SGMCMC_LANCZOS_MAX_M;
constexpr int kMaxSplits = SGMCMC_LANCZOS_MAX_SPLITS;
constexpr int kMaxBatch = SGMCMC_LANCZOS_MAX_BATCH;
constexpr int kWidth = SGMCMC_LANCZOS_WIDTH;            // doubles of one workgroup's partials: c[kMaxM], |w|^2, non-finite
constexpr int kNorm = kMaxM, kBad = kMaxM + 1;
constexpr int kState = SGMCMC_LANCZOS_STATE;            // scale, 1 / beta, beta, breakdown, non-finite, norm before
constexpr int kMaxSweeps = SGMCMC_TRIDIAG_MAX_SWEEPS;
constexpr int kAhead = 8;                               // rows of the eigenvector matrix a thread loads ahead of its stores
constexpr int64_t kMaxD = ((int64_t)1 << 31) - 1;
constexpr int kRitzCoords = 64, kRitzCols = 16, kRitzK = 32, kRitzStride = kRitzCoords + 16;
static_assert(kChunk == kThreads && kWidth >= kMaxM + 2 && kState >= 6 && kMaxM % kThreads == 0, "step geometry");
using gram::f64x4;

inline int64_t chunks_of(int64_t D) { return (D + kChunk - 1) / kChunk; }
inline bool shape_ok(int64_t D) { return D >= 1 && D <= kMaxD; }
inline int splits(int64_t D, int64_t workspace_bytes) {
  int64_t s = chunks_of(D);
  if (s > kMaxSplits) s = kMaxSplits;
  const int64_t fit = workspace_bytes / ((int64_t)sizeof(double) * kWidth);
  if (s > fit) s = fit;
  return (int)(s < 0 ? 0 : s);
}

// lane l += lane l + 32, ..., l + 1: lane 0 of a wave holds the wave's sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_down(v, off, 64));
  return v;
}

// the workgroup's sum: the waves' sums added from wave 0 upwards; valid in thread 0.  sh: kThreads / 64 doubles per value
__device__ __forceinline__ double block_sum4(double v, double* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int q = 1; q < kThreads / 64; ++q) s = __dadd_rn(s, sh[q]);
  __syncthreads();
  return s;
}

// ---- 1. dots: ws[split][k] = the workgroup's part of V_k . w for its kRows rows; the first row tile also |w|^2 and the
//         non-finite elements of w -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dots_kernel(const double* __restrict__ V, int64_t vs, int nrows,
                                                        const double* __restrict__ w, int64_t D, int64_t nchunks,
                                                        double* __restrict__ ws) {
  __shared__ double sh[kThreads / 64];
  const int t = threadIdx.x, split = blockIdx.x, nsplit = gridDim.x, r0 = blockIdx.y * kRows;
  const int nr = nrows - r0 < kRows ? nrows - r0 : kRows;
  double acc[kRows], nrm = 0.0, bad = 0.0;
#pragma unroll
  for (int r = 0; r < kRows; ++r) acc[r] = 0.0;
  for (int64_t c = split; c < nchunks; c += nsplit) {
    const int64_t col = c * kChunk + t;
    if (col < D) {
      const double wv = w[col];
      nrm = fma(wv, wv, nrm);
      bad += num::is_finite(wv) ? 0.0 : 1.0;
      const double* v = V + (int64_t)r0 * vs + col;
#pragma unroll
      for (int r = 0; r < kRows; ++r)
        if (r < nr) acc[r] = fma(v[(int64_t)r * vs], wv, acc[r]);
    }
  }
  double* out = ws + (size_t)split * kWidth;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const double s = block_sum4(acc[r], sh);
    if (t == 0 && r < nr) out[r0 + r] = s;
  }
  if (blockIdx.y == 0) {
    const double n = block_sum4(nrm, sh), b = block_sum4(bad, sh);
    if (t == 0) out[kNorm] = n, out[kBad] = b;
  }
}

// ---- 2. reduce: the workgroups' partials added from 0 upwards; pass 0 / 1: the coefficients of a Gram-Schmidt pass, pass 2:
//         alpha_j, beta_j, scale, the breakdown flag and 1 / beta ------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void reduce_kernel(const double* __restrict__ ws, int splits, int nrows, int pass, int j,
                                                          int restart, double rtol, double* __restrict__ coef,
                                                          double* __restrict__ alpha, double* __restrict__ beta,
                                                          double* __restrict__ state) {
  const int t = threadIdx.x;
  if (pass < 2) {
    for (int k = t; k < nrows; k += kThreads) {
      double s = 0.0;
      for (int q = 0; q < splits; ++q) s = __dadd_rn(s, ws[(size_t)q * kWidth + k]);
      coef[pass * kMaxM + k] = s;
    }
    if (t == 0) {
      double n = 0.0, b = 0.0;
      for (int q = 0; q < splits; ++q) {
        n = __dadd_rn(n, ws[(size_t)q * kWidth + kNorm]);
        b += ws[(size_t)q * kWidth + kBad];
      }
      state[4] += b;
      if (pass == 0) state[5] = sqrt(n);
    }
    return;
  }
  if (t != 0) return;
  double n = 0.0;
  for (int q = 0; q < splits; ++q) n = __dadd_rn(n, ws[(size_t)q * kWidth + kNorm]);
  const double b = sqrt(n);
  bool ok;
  if (restart) {
    ok = b > rtol * state[5];
  } else {
    const double a = coef[j] + coef[kMaxM + j];
    double scale = state[0];
    if (fabs(a) > scale) scale = fabs(a);
    if (b > scale) scale = b;
    ok = b > rtol * scale;
    alpha[j] = a;
    beta[j] = ok ? b : (b == b ? 0.0 : b);              // (a NaN norm stays NaN: the host reads the non-finite count)
    state[0] = scale;
  }
  state[1] = ok ? 1.0 / b : 0.0;
  state[2] = b;
  state[3] = ok ? 0.0 : 1.0;
}

// ---- 3. update: mode 0: w -= sum_k c_k V_k, k ascending, an fma per term, and ws[split][kNorm] = the workgroup's part of
//         |w|^2 afterwards; mode 1: v_next = w / beta (as w * state[1]) ------------------------------------------------------
__global__ __launch_bounds__(kThreads) void update_kernel(const double* __restrict__ V, int64_t vs, int nrows,
                                                          double* __restrict__ w, int64_t D, int64_t nchunks,
                                                          const double* __restrict__ coef, int mode,
                                                          const double* __restrict__ state, double* __restrict__ v_next,
                                                          double* __restrict__ ws) {
  __shared__ double sh[kThreads / 64];
  const int t = threadIdx.x, split = blockIdx.x, nsplit = gridDim.x;
  if (mode == 1) {
    const double inv = state[1];
    for (int64_t c = split; c < nchunks; c += nsplit) {
      const int64_t col = c * kChunk + t;
      if (col < D) v_next[col] = w[col] * inv;
    }
    return;
  }
  double nrm = 0.0;
  for (int64_t c = split; c < nchunks; c += nsplit) {
    const int64_t col = c * kChunk + t;
    if (col < D) {
      double wv = w[col];
      const double* v = V + col;
#pragma unroll 4
      for (int k = 0; k < nrows; ++k) wv = fma(-coef[k], v[(int64_t)k * vs], wv);
      w[col] = wv;
      nrm = fma(wv, wv, nrm);
    }
  }
  const double n = block_sum4(nrm, sh);
  if (t == 0) ws[(size_t)split * kWidth + kNorm] = n;
}

// ---- 4. tridiagonal eigensolver: one workgroup per matrix; d, e and a sweep's rotations in LDS; thread 0 runs the QL
//         recurrence, every thread applies the rotations to the rows k = t, t + 256 of the eigenvector matrix, kept in global
//         memory as work[i][k] = Z[k][i] so that a wave's rows are contiguous ------------------------------------------------
__global__ __launch_bounds__(kThreads) void tridiag_kernel(const double* __restrict__ alpha, const double* __restrict__ beta,
                                                           int m, int64_t ld, double* __restrict__ theta,
                                                           double* __restrict__ Y, double* __restrict__ work,
                                                           int* __restrict__ sweeps, int* __restrict__ failed) {
  __shared__ double sd[kMaxM], se[kMaxM], sc[kMaxM], ss[kMaxM];
  __shared__ int sperm[kMaxM];
  __shared__ int ctl[4];                                // hi (exclusive top rotation + 1), lo, status, sweep count
  const int t = threadIdx.x, b = blockIdx.x;
  const double* a_in = alpha + (int64_t)b * ld;
  const double* b_in = beta + (int64_t)b * ld;
  double* Z = work + (size_t)b * m * m;
  double* Yb = Y + (size_t)b * m * m;
  for (int i = t; i < m; i += kThreads) {
    sd[i] = a_in[i];
    se[i] = i + 1 < m ? b_in[i] : 0.0;
  }
  for (int idx = t; idx < m * m; idx += kThreads) Z[idx] = (idx / m == idx % m) ? 1.0 : 0.0;
  if (t == 0) ctl[3] = 0;
  __syncthreads();
  constexpr double eps = 2.220446049250313e-16;
  bool fail = false;
  for (int l = 0; l < m && !fail; ++l) {
    for (int iter = 0;; ++iter) {
      if (t == 0) {
        int mm = l;
        for (; mm < m - 1; ++mm) {
          const double dd = fabs(sd[mm]) + fabs(sd[mm + 1]);
          if (fabs(se[mm]) <= eps * dd) break;
        }
        if (mm == l) {
          ctl[2] = 0;                                   // deflated: the next l
        } else if (iter == kMaxSweeps) {
          ctl[2] = 2;                                   // not deflated after kMaxSweeps sweeps
        } else {
          ctl[2] = 1;
          ctl[3] += 1;
          double g = (sd[l + 1] - sd[l]) / (2.0 * se[l]);
          double r = hypot(g, 1.0);
          g = sd[mm] - sd[l] + se[l] / (g + copysign(r, g));
          double s = 1.0, c = 1.0, p = 0.0;
          int i = mm - 1;
          for (; i >= l; --i) {
            const double f = s * se[i], bb = c * se[i];
            r = hypot(f, g);
            se[i + 1] = r;
            if (r == 0.0) {
              sd[i + 1] -= p;
              se[mm] = 0.0;
              break;
            }
            s = f / r;
            c = g / r;
            g = sd[i + 1] - p;
            r = (sd[i] - g) * s + 2.0 * c * bb;
            p = s * r;
            sd[i + 1] = g + p;
            g = c * r - bb;
            sc[i] = c;
            ss[i] = s;
          }
          if (i < l) {
            sd[l] -= p;
            se[l] = g;
            se[mm] = 0.0;
          }
          ctl[0] = mm;
          ctl[1] = i + 1;                               // rotations mm - 1 .. i + 1 were formed
        }
      }
      __syncthreads();
      const int status = ctl[2], hi = ctl[0], lo = ctl[1];
      if (status == 1) {
        for (int k = t; k < m; k += kThreads) {
          double f = Z[(size_t)hi * m + k];
          int i = hi - 1;
          for (; i - (kAhead - 1) >= lo; i -= kAhead) {   // kAhead loads in flight before the first store (same arithmetic)
            double z[kAhead];
#pragma unroll
            for (int q = 0; q < kAhead; ++q) z[q] = Z[(size_t)(i - q) * m + k];
#pragma unroll
            for (int q = 0; q < kAhead; ++q) {
              const double c = sc[i - q], s = ss[i - q];
              Z[(size_t)(i - q + 1) * m + k] = s * z[q] + c * f;
              f = c * z[q] - s * f;
            }
          }
          for (; i >= lo; --i) {
            const double zi = Z[(size_t)i * m + k], c = sc[i], s = ss[i];
            Z[(size_t)(i + 1) * m + k] = s * zi + c * f;
            f = c * zi - s * f;
          }
          Z[(size_t)lo * m + k] = f;
        }
      }
      __syncthreads();
      if (status == 0) break;
      if (status == 2) {
        fail = true;
        break;
      }
    }
  }
  // theta ascending, ties by index: the rank of every eigenvalue, then the columns in that order
  for (int i = t; i < m; i += kThreads) {
    const double di = sd[i];
    int rank = 0;
    for (int q = 0; q < m; ++q) rank += sd[q] < di || (sd[q] == di && q < i);
    if (!(di == di)) fail = true;
    sperm[fail ? i : rank] = i;
  }
  ctl[2] = 0;
  __syncthreads();
  if (fail) ctl[2] = 1;                                 // (a NaN eigenvalue one thread saw: everybody's failure)
  __syncthreads();
  fail = ctl[2] != 0;
  for (int p = t; p < m; p += kThreads) theta[(int64_t)b * ld + p] = fail ? num::qnan() : sd[sperm[p]];
  for (int idx = t; idx < m * m; idx += kThreads) {
    const int k = idx / m, p = idx - k * m;
    Yb[idx] = fail ? num::qnan() : Z[(size_t)sperm[p] * m + k];
  }
  if (t == 0) {
    sweeps[b] = ctl[3];
    failed[b] = fail ? 1 : 0;
  }
}

// ---- 5. Ritz vectors: U [D][k] = V^T Y[:, col0 .. col0 + k), the sum over the m rows in ascending groups of four on the
//         fp64 matrix pipe; a wave forms 16 coordinates x 16 columns, a workgroup 64 coordinates ----------------------------
__global__ __launch_bounds__(kThreads) void ritz_kernel(const double* __restrict__ V, int64_t vs, int m, int64_t D,
                                                        const double* __restrict__ Y, const double* __restrict__ theta,
                                                        int col0, int k, int positive, double* __restrict__ U) {
  __shared__ double sV[kRitzK * kRitzStride];
  __shared__ double sY[kRitzK * kRitzCols];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t cb = (int64_t)blockIdx.x * kRitzCoords;
  const int jb = blockIdx.y * kRitzCols;
  f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int rb = 0; rb < m; rb += kRitzK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kRitzK * kRitzCoords / kThreads; ++i) {
      const int r = (t >> 6) + 4 * i;
      const int64_t col = cb + (t & 63);
      sV[r * kRitzStride + (t & 63)] = (rb + r < m && col < D) ? V[(int64_t)(rb + r) * vs + col] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kRitzK * kRitzCols / kThreads; ++i) {
      const int r = (t >> 4) + 16 * i, j = jb + (t & 15);
      sY[r * kRitzCols + (t & 15)] = (rb + r < m && j < k) ? Y[(size_t)(rb + r) * m + col0 + j] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kRitzK; kk += 4) {
      const double a = sV[(kk + (lane >> 4)) * kRitzStride + wave * 16 + (lane & 15)];
      const double bv = sY[(kk + (lane >> 4)) * kRitzCols + (lane & 15)];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc, 0, 0, 0);
    }
  }
  const int j = jb + (lane & 15);
  if (j >= k) return;
  const double top = fmax(fabs(theta[0]), fabs(theta[m - 1]));
  const bool zero = positive && theta[col0 + j] <= (double)m * 2.220446049250313e-16 * top;
  const double sign = Y[col0 + j] >= 0.0 ? 1.0 : -1.0;   // (row 0 of Y: the component along the start vector)
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t col = cb + wave * 16 + (lane >> 4) + 4 * reg;
    if (col < D) U[(size_t)col * k + j] = zero ? 0.0 : sign * acc[reg];
  }
}

// ---- 6. N_eff: out[b][a] = sum over eigs[b][i] > 0 of eigs / (eigs + alpha_a), compensated; thread t adds i = t, t + 256,
//         ..., thread 0 then adds the threads' sums from 0 upwards ---------------------------------------------------------
__global__ __launch_bounds__(kThreads) void effdim_kernel(const double* __restrict__ eigs, int k,
                                                          const double* __restrict__ alphas, int A, double* __restrict__ out,
                                                          long long* __restrict__ nonpos, long long* __restrict__ nonfinite) {
  __shared__ double sS[kThreads], sC[kThreads];
  __shared__ int sN[kThreads], sF[kThreads];
  const int t = threadIdx.x, a = blockIdx.y;
  const int64_t b = blockIdx.x;
  const double* e = eigs + b * (int64_t)k;
  const double al = alphas[a];
  double s = 0.0, c = 0.0;
  int np = 0, nf = 0;
  for (int i = t; i < k; i += kThreads) {
    const double v = e[i];
    if (!num::is_finite(v)) ++nf;
    else if (!(v > 0.0)) ++np;
    else num::comp_add(s, c, v / (v + al));
  }
  sS[t] = s, sC[t] = c, sN[t] = np, sF[t] = nf;
  __syncthreads();
  if (t != 0) return;
  double S = 0.0, C = 0.0;
  long long NP = 0, NF = 0;
  for (int q = 0; q < kThreads; ++q) {
    num::comp_add(S, C, sS[q]);
    C += sC[q];
    NP += sN[q];
    NF += sF[q];
  }
  out[b * A + a] = S + C;
  if (a == 0) nonpos[b] = NP, nonfinite[b] = NF;
}

}  // namespace lanczos

extern "C" int sgmcmc_lanczos_splits(int64_t D, int64_t workspace_bytes) {
  if (!lanczos::shape_ok(D) || workspace_bytes < 0) return -1;
  return lanczos::splits(D, workspace_bytes);
}

extern "C" int64_t sgmcmc_lanczos_workspace_bytes(int64_t D, int64_t workspace_bytes) {
  if (!lanczos::shape_ok(D) || workspace_bytes < 0) return -1;
  return (int64_t)lanczos::splits(D, workspace_bytes) * lanczos::kWidth * (int64_t)sizeof(double);
}

extern "C" int sgmcmc_lanczos_dots(const double* V, int64_t v_stride, int nrows, const double* w, int64_t D, int splits,
                                   double* ws, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!V || !w || !ws || !lanczos::shape_ok(D) || v_stride < 0 || nrows < 1 || nrows > lanczos::kMaxM || splits < 1 ||
      splits > lanczos::kMaxSplits || splits > lanczos::chunks_of(D))
    return (int)hipErrorInvalidValue;
  const dim3 grid(splits, (nrows + lanczos::kRows - 1) / lanczos::kRows);
  SGMCMC_LAUNCH(lanczos::dots_kernel, grid, dim3(lanczos::kThreads), 0, (hipStream_t)stream, V, v_stride, nrows, w, D,
                lanczos::chunks_of(D), ws);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_lanczos_reduce(const double* ws, int splits, int nrows, int pass, int j, int restart, double rtol,
                                     double* coef, double* alpha, double* beta, double* state, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!ws || !coef || !state || splits < 1 || splits > lanczos::kMaxSplits || nrows < 1 || nrows > lanczos::kMaxM ||
      pass < 0 || pass > 2 || !(rtol >= 0.0) || (pass == 2 && !restart && (!alpha || !beta || j < 0 || j >= nrows)))
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(lanczos::reduce_kernel, dim3(1), dim3(lanczos::kThreads), 0, (hipStream_t)stream, ws, splits, nrows, pass, j,
                restart, rtol, coef, alpha, beta, state);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_lanczos_update(const double* V, int64_t v_stride, int nrows, double* w, int64_t D, int splits,
                                     const double* coef, int mode, const double* state, double* v_next, double* ws,
                                     void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!w || !lanczos::shape_ok(D) || splits < 1 || splits > lanczos::kMaxSplits || splits > lanczos::chunks_of(D) ||
      (mode != 0 && mode != 1) || (mode == 0 && (!V || !coef || !ws || v_stride < 0 || nrows < 1 || nrows > lanczos::kMaxM)) ||
      (mode == 1 && (!state || !v_next)))
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(lanczos::update_kernel, dim3(splits), dim3(lanczos::kThreads), 0, (hipStream_t)stream, V, v_stride, nrows, w,
                D, lanczos::chunks_of(D), coef, mode, state, v_next, ws);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_tridiag_eig(const double* alpha, const double* beta, int batch, int m, int64_t ld, double* theta,
                                  double* Y, double* work, int* sweeps, int* failed, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!alpha || !beta || !theta || !Y || !work || !sweeps || !failed || batch < 1 || batch > lanczos::kMaxBatch || m < 1 ||
      m > lanczos::kMaxM || ld < m)
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(lanczos::tridiag_kernel, dim3(batch), dim3(lanczos::kThreads), 0, (hipStream_t)stream, alpha, beta, m, ld,
                theta, Y, work, sweeps, failed);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_lanczos_ritz(const double* V, int64_t v_stride, int m, int64_t D, const double* Y, const double* theta,
                                   int col0, int k, int positive, double* U, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!V || !Y || !theta || !U || !lanczos::shape_ok(D) || v_stride < 0 || m < 1 || m > lanczos::kMaxM || col0 < 0 ||
      k < 1 || col0 + k > m)
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((D + lanczos::kRitzCoords - 1) / lanczos::kRitzCoords),
                  (k + lanczos::kRitzCols - 1) / lanczos::kRitzCols);
  SGMCMC_LAUNCH(lanczos::ritz_kernel, grid, dim3(lanczos::kThreads), 0, (hipStream_t)stream, V, v_stride, m, D, Y, theta, col0,
                k, positive, U);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_effdim(const double* eigs, int64_t B, int k, const double* alphas, int A, double* out, int64_t* nonpos,
                             int64_t* nonfinite, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!eigs || !alphas || !out || !nonpos || !nonfinite || B < 1 || B > ((int64_t)1 << 31) - 1 || k < 1 || A < 1 ||
      A > lanczos::kMaxBatch)
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(lanczos::effdim_kernel, dim3((unsigned)B, A), dim3(lanczos::kThreads), 0, (hipStream_t)stream, eigs, k,
                alphas, A, out, (long long*)nonpos, (long long*)nonfinite);
  return (int)hipGetLastError();
}
