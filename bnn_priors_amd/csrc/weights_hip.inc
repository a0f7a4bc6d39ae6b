// Model-averaging weights from the pointwise elpd table P[k][i] of K models x N observations (Yao, Vehtari, Simpson,
// Gelman 2018): stacking of predictive distributions, pseudo-BMA, pseudo-BMA+ (Bayesian bootstrap) and the log density
// of a weighted mixture.  include/sgmcmc_hip.h states the definition; this is the device path.
//
//   slice_kernel      one workgroup per slice of 1,024 observations, lane = observation (thread t owns observations
//                     t, t + 256, t + 512, t + 768 of its slice, ascending), so a model's row is read coalesced.
//                     Three modes: stacking (sum q / mix per model and sum (m + log mix)), mixture (the pointwise row and
//                     sum (m + log mix) for a given w) and row sums (pseudo-BMA).  Writes its row of part [slices][K + 1].
//   stack_finish      one workgroup: the slices in ascending order, r, gap, lpd and the iteration counter into the state
//                     record, then w <- w r unless the state is frozen (converged, at max_iter, or non-finite input).
//                     A frozen state makes both kernels of a pair return at once.
//   boot_kernel       grid = slices x replicates; thread t owns quad t of its slice (observations 4t .. 4t + 3): one
//                     Philox call per four observations; part [replicates][slices][K + 1] of sum g P[k] and sum g
//   boot_row_kernel   one thread per replicate: the slices in ascending order, z, softmax
//   boot_total_kernel one workgroup: the means of w and the two-pass standard deviation of z over the replicates
//
// Every per-slice sum is 256 partial sums (one per thread, its observations in ascending order) and a fixed tree
// (thread t adds t + 128, then t + 64, ...); the slices are added in ascending order.  No atomics.  A non-finite entry of
// P makes the last column of its slice's partials NaN, which the finishing kernels turn into NaN everywhere.

namespace weights {

constexpr int kSlice = SGMCMC_WEIGHTS_SLICE;
constexpr int kT = 256;
constexpr int kPer = kSlice / kT;
constexpr int kMaxK = SGMCMC_WEIGHTS_MAX_MODELS;
constexpr uint32_t kPurpose = SGMCMC_WEIGHTS_NOISE_PURPOSE;
enum { sIter, sConverged, sFrozen, sGap, sLpd, sTol, sMaxIter, sReserved, sW, sR = sW + kMaxK };
static_assert(sR + kMaxK == SGMCMC_WEIGHTS_STATE && kPer * kT == kSlice && kPer == 4, "state record, slice geometry");

enum { kStack, kMix, kRowSum };

inline bool valid_shape(int K, int64_t N, int64_t stride) {
  return K >= 1 && K <= kMaxK && N >= 1 && stride >= N && (N + kSlice - 1) / kSlice <= 0x7fffffffll;
}
inline int64_t slices_of(int64_t N) { return (N + kSlice - 1) / kSlice; }
inline int64_t stack_bytes(int K, int64_t N, bool cache_q) {
  return 8 * (slices_of(N) * (K + 1) + (cache_q ? (int64_t)(K + 1) * N : 0));
}
inline int64_t replicate_bytes(int K, int64_t N) { return 8 * slices_of(N) * (K + 1); }

// rows [K][kT] of per-thread partial sums in LDS -> row k's total in sh[k * kT]; ends with a barrier
__device__ __forceinline__ void reduce_rows(double* sh, int K) {
  for (int w = kT / 2; w > 0; w /= 2) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < K * w; idx += kT) {
      const int at = (idx / w) * kT + idx % w;
      sh[at] = __dadd_rn(sh[at], sh[at + w]);
    }
  }
  __syncthreads();
}

// the totals of the first `rows` (K or none) rows into out[0 .. rows - 1], the scalar's total into out[K]
__device__ __forceinline__ void finish_slice(double* sh, int rows, int K, double scal, double* __restrict__ out) {
  const int tid = threadIdx.x;
  reduce_rows(sh, rows);
  if (tid < rows) out[tid] = sh[tid * kT];
  __syncthreads();
  sh[tid] = scal;
  reduce_rows(sh, 1);
  if (tid == 0) out[K] = sh[0];
}

// cache: m [N] (NaN for a column with a non-finite entry), then q [K][N]
template <int MODE, bool CACHED>
__global__ __launch_bounds__(kT) void slice_kernel(const double* __restrict__ P, int64_t stride, int K, int64_t N,
                                                   const double* __restrict__ w, const double* __restrict__ state,
                                                   const double* __restrict__ cache, double* __restrict__ part,
                                                   double* __restrict__ pointwise) {
  __shared__ double sh[kMaxK * kT];
  if (MODE == kStack && state[sFrozen] != 0.0) return;
  const int tid = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * kSlice + tid;
  // the thread's observations: i[j] = first + j * 256 for j < n; the four are walked side by side (independent loads,
  // exponentials and divisions in flight) and added in ascending j, a slot past the end repeats the last valid one
  const int n = first >= N ? 0 : (int)((N - first + kT - 1) / kT < kPer ? (N - first + kT - 1) / kT : kPer);
  int64_t i[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) i[j] = first + (int64_t)(j < n ? j : (n > 0 ? n - 1 : 0)) * kT;
  double scal = 0.0;
  if (n == 0) {
    if (MODE != kMix)
      for (int k = 0; k < K; ++k) sh[k * kT + tid] = 0.0;
  } else if (MODE == kRowSum) {
    bool finite = true;
    for (int k = 0; k < K; ++k) {
      const double* __restrict__ row = P + (int64_t)k * stride;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const double v = row[i[j]];
        finite = finite && fabs(v) < INFINITY;
        acc = j < n ? __dadd_rn(acc, v) : acc;
      }
      sh[k * kT + tid] = acc;
    }
    scal = finite ? 0.0 : NAN;
  } else {
    double m[kPer], mix[kPer];
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < kPer; ++j) m[j] = cache[i[j]];
    } else {
      bool finite[kPer];
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        m[j] = -INFINITY;
        finite[j] = true;
      }
      for (int k = 0; k < K; ++k) {
        const double* __restrict__ row = P + (int64_t)k * stride;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const double v = row[i[j]];
          finite[j] = finite[j] && fabs(v) < INFINITY;
          m[j] = v > m[j] ? v : m[j];
        }
      }
#pragma unroll
      for (int j = 0; j < kPer; ++j) m[j] = finite[j] ? m[j] : NAN;
    }
#define WEIGHTS_Q(k, j) \
  (CACHED ? cache[(int64_t)((k) + 1) * N + i[j]] : exp(__dsub_rn(P[(int64_t)(k) * stride + i[j]], m[j])))
#pragma unroll
    for (int j = 0; j < kPer; ++j) mix[j] = 0.0;
    for (int k = 0; k < K; ++k) {
      const double wk = w[k];
#pragma unroll
      for (int j = 0; j < kPer; ++j) mix[j] = __dadd_rn(mix[j], __dmul_rn(wk, WEIGHTS_Q(k, j)));
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const double lm = __dadd_rn(m[j], log(mix[j]));
      if (j < n) {
        scal = __dadd_rn(scal, lm);
        if (MODE == kMix) pointwise[i[j]] = lm;
      }
    }
    if (MODE == kStack)
      for (int k = 0; k < K; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const double v = WEIGHTS_Q(k, j) / mix[j];
          acc = j < n ? __dadd_rn(acc, v) : acc;
        }
        sh[k * kT + tid] = acc;
      }
#undef WEIGHTS_Q
  }
  finish_slice(sh, MODE == kMix ? 0 : K, K, scal, part + (int64_t)blockIdx.x * (K + 1));
}

// the state record, and (cache != NULL) m and q of every observation
__global__ __launch_bounds__(kT) void stack_init_kernel(const double* __restrict__ P, int64_t stride, int K, int64_t N,
                                                        double tol, double max_iter, double* __restrict__ state,
                                                        double* __restrict__ cache) {
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid < SGMCMC_WEIGHTS_STATE) {
    double v = 0.0;
    if (tid == sTol) v = tol;
    if (tid == sMaxIter) v = max_iter;
    if (tid == sGap || tid == sLpd) v = NAN;
    if (tid >= sW && tid < sW + K) v = 1.0 / (double)K;
    state[tid] = v;
  }
  if (!cache) return;
  const int64_t i = (int64_t)blockIdx.x * kT + tid;
  if (i >= N) return;
  bool finite = true;
  double m = -INFINITY;
  for (int k = 0; k < K; ++k) {
    const double v = P[(int64_t)k * stride + i];
    finite = finite && fabs(v) < INFINITY;
    m = v > m ? v : m;
  }
  m = finite ? m : NAN;
  cache[i] = m;
  for (int k = 0; k < K; ++k) cache[(int64_t)(k + 1) * N + i] = exp(__dsub_rn(P[(int64_t)k * stride + i], m));
}

__global__ __launch_bounds__(64) void stack_finish_kernel(const double* __restrict__ part, int64_t slices, int K,
                                                          int64_t N, double* __restrict__ state) {
  __shared__ double r[kMaxK + 1];
  if (state[sFrozen] != 0.0) return;
  const int tid = threadIdx.x;
  const double tol = state[sTol], max_iter = state[sMaxIter], it = state[sIter];
  if (tid <= K) {
    double a = 0.0;
    for (int64_t s = 0; s < slices; ++s) a = __dadd_rn(a, part[s * (K + 1) + tid]);
    r[tid] = tid < K ? a / (double)N : a;
  }
  __syncthreads();
  const double lpd = r[K];
  const bool bad = lpd != lpd;
  double mx = r[0];
  for (int k = 1; k < K; ++k) mx = r[k] > mx ? r[k] : mx;
  const double gap = __dsub_rn(mx, 1.0);
  const bool converged = !bad && gap <= tol;
  const bool stop = bad || converged || it >= max_iter;
  if (tid < K) {
    state[sR + tid] = bad ? NAN : r[tid];
    if (bad) state[sW + tid] = NAN;
    else if (!stop) state[sW + tid] = __dmul_rn(state[sW + tid], r[tid]);
  }
  if (tid == 0) {
    state[sGap] = bad ? NAN : gap;
    state[sLpd] = lpd;
    if (stop) {
      state[sConverged] = converged ? 1.0 : 0.0;
      state[sFrozen] = 1.0;
    } else {
      state[sIter] = __dadd_rn(it, 1.0);
    }
  }
}

__global__ __launch_bounds__(64) void mix_finish_kernel(const double* __restrict__ part, int64_t slices, int K,
                                                        double* __restrict__ total) {
  if (threadIdx.x != 0) return;
  double a = 0.0;
  for (int64_t s = 0; s < slices; ++s) a = __dadd_rn(a, part[s * (K + 1) + K]);
  total[0] = a;
}

// out [2][K]: the weights, then elpd_k
__global__ __launch_bounds__(64) void bma_finish_kernel(const double* __restrict__ part, int64_t slices, int K,
                                                        double* __restrict__ out) {
  __shared__ double e[kMaxK + 1];
  const int tid = threadIdx.x;
  if (tid <= K) {
    double a = 0.0;
    for (int64_t s = 0; s < slices; ++s) a = __dadd_rn(a, part[s * (K + 1) + tid]);
    e[tid] = a;
  }
  __syncthreads();
  if (tid >= K) return;
  const bool bad = e[K] != e[K];
  double mx = e[0];
  for (int k = 1; k < K; ++k) mx = e[k] > mx ? e[k] : mx;
  double den = 0.0;
  for (int k = 0; k < K; ++k) den = __dadd_rn(den, exp(__dsub_rn(e[k], mx)));
  out[tid] = bad ? NAN : exp(__dsub_rn(e[tid], mx)) / den;
  out[K + tid] = bad ? NAN : e[tid];
}

__global__ __launch_bounds__(kT) void boot_kernel(const double* __restrict__ P, int64_t stride, int K, int64_t N,
                                                  uint64_t seed, uint32_t stream, int64_t b0, int64_t slices,
                                                  double* __restrict__ part) {
  __shared__ double sh[kMaxK * kT];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kSlice + 4 * tid;
  const uint64_t draw = (uint64_t)(b0 + blockIdx.y), quad = (uint64_t)i0 >> 2;
  double scal = 0.0;
  if (i0 >= N) {
    for (int k = 0; k < K; ++k) sh[k * kT + tid] = 0.0;
  } else {
    uint32_t x[4];
    philox4x32_10((uint32_t)quad, (uint32_t)(quad >> 32), (uint32_t)draw,
                  (kPurpose << 28) | ((stream & 0xFFFu) << 16) | (uint32_t)((draw >> 32) & 0xFFFFu), (uint32_t)seed,
                  (uint32_t)(seed >> 32), x);
    const int n = N - i0 < 4 ? (int)(N - i0) : 4;
    double g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      g[j] = -log((double)spec_uniform(x[j]));
      scal = j < n ? __dadd_rn(scal, g[j]) : scal;
    }
    bool finite = true;
    for (int k = 0; k < K; ++k) {
      const double* __restrict__ row = P + (int64_t)k * stride;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double v = row[i0 + (j < n ? j : n - 1)];
        finite = finite && fabs(v) < INFINITY;
        acc = j < n ? __dadd_rn(acc, __dmul_rn(g[j], v)) : acc;
      }
      sh[k * kT + tid] = acc;
    }
    scal = finite ? scal : NAN;
  }
  finish_slice(sh, K, K, scal, part + ((int64_t)blockIdx.y * slices + blockIdx.x) * (K + 1));
}

// z, w [B][K]: rows b0 .. b0 + count - 1
__global__ __launch_bounds__(64) void boot_row_kernel(const double* __restrict__ part, int64_t slices, int K, int64_t N,
                                                      int64_t b0, int64_t count, double* __restrict__ z,
                                                      double* __restrict__ w) {
  const int64_t bl = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (bl >= count) return;
  const double* __restrict__ p = part + bl * slices * (K + 1);
  double* __restrict__ zr = z + (b0 + bl) * K;
  double* __restrict__ wr = w + (b0 + bl) * K;
  double G = 0.0;
  for (int64_t s = 0; s < slices; ++s) G = __dadd_rn(G, p[s * (K + 1) + K]);
  double mx = -INFINITY;
  for (int k = 0; k < K; ++k) {
    double X = 0.0;
    for (int64_t s = 0; s < slices; ++s) X = __dadd_rn(X, p[s * (K + 1) + k]);
    const double v = G != G ? NAN : __dmul_rn((double)N, X) / G;
    zr[k] = v;
    mx = v > mx ? v : mx;
  }
  double den = 0.0;
  for (int k = 0; k < K; ++k) den = __dadd_rn(den, exp(__dsub_rn(zr[k], mx)));
  for (int k = 0; k < K; ++k) wr[k] = exp(__dsub_rn(zr[k], mx)) / den;
}

// out [2][K]: mean_b w, then sqrt(var_b z) with ddof 1 in two passes; sums over b as num::block_sum takes them
__global__ __launch_bounds__(kT) void boot_total_kernel(const double* __restrict__ z, const double* __restrict__ w,
                                                        int64_t B, int K, double* __restrict__ out) {
  __shared__ double sh[kT];
  const double dB = (double)B;
  for (int k = 0; k < K; ++k) {
    const double mw = num::block_sum<kT>(B, sh, [&](int64_t b) { return w[b * K + k]; }) / dB;
    const double mz = num::block_sum<kT>(B, sh, [&](int64_t b) { return z[b * K + k]; }) / dB;
    const double ssq = num::block_sum<kT>(B, sh, [&](int64_t b) {
      const double d = __dsub_rn(z[b * K + k], mz);
      return __dmul_rn(d, d);
    });
    if (threadIdx.x == 0) {
      out[k] = mw;
      out[K + k] = sqrt(ssq / __dsub_rn(dB, 1.0));
    }
  }
}

inline bool valid_call(const void* P, int64_t stride, int K, int64_t N, const void* workspace, int64_t bytes,
                       int64_t need) {
  return P && workspace && (uintptr_t)workspace % 8 == 0 && valid_shape(K, N, stride) && bytes >= need;
}

}  // namespace weights

extern "C" int64_t sgmcmc_weights_workspace_bytes(int models, int64_t observations, int64_t replicates, int cache_q) {
  if (!weights::valid_shape(models, observations, observations) || replicates < 0) return -1;
  const int64_t stack = weights::stack_bytes(models, observations, cache_q != 0);
  if (replicates > INT64_MAX / weights::replicate_bytes(models, observations)) return -1;
  const int64_t boot = replicates * weights::replicate_bytes(models, observations);
  return stack > boot ? stack : boot;
}

extern "C" int sgmcmc_stacking_init(const double* P, int64_t model_stride, int models, int64_t observations, double tol,
                                    int64_t max_iter, int cache_q, void* workspace, int64_t workspace_bytes,
                                    double* state, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const int K = models;
  const int64_t N = observations;
  if (!state || !(tol >= 0.0) || max_iter < 0 || max_iter > (1ll << 52) ||
      !weights::valid_call(P, model_stride, K, N, workspace, workspace_bytes, weights::stack_bytes(K, N, cache_q != 0)))
    return (int)hipErrorInvalidValue;
  double* cache = cache_q ? (double*)workspace + weights::slices_of(N) * (K + 1) : nullptr;
  const int64_t blocks = cache_q ? (N + weights::kT - 1) / weights::kT : 1;
  if (blocks > 0x7fffffffll) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(weights::stack_init_kernel, dim3((unsigned)blocks), dim3(weights::kT), 0, (hipStream_t)stream, P,
                model_stride, K, N, tol, (double)max_iter, state, cache);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_stacking_iterate(const double* P, int64_t model_stride, int models, int64_t observations,
                                       int cache_q, int iters, void* workspace, int64_t workspace_bytes, double* state,
                                       void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const int K = models;
  const int64_t N = observations;
  if (!state || iters < 0 ||
      !weights::valid_call(P, model_stride, K, N, workspace, workspace_bytes, weights::stack_bytes(K, N, cache_q != 0)))
    return (int)hipErrorInvalidValue;
  const int64_t slices = weights::slices_of(N);
  double* part = (double*)workspace;
  const double* cache = cache_q ? part + slices * (K + 1) : nullptr;
  const dim3 grid((unsigned)slices), block(weights::kT);
  hipStream_t s = (hipStream_t)stream;
  for (int t = 0; t < iters; ++t) {
    if (cache_q) SGMCMC_LAUNCH((weights::slice_kernel<weights::kStack, true>), grid, block, 0, s, P, model_stride, K,
                               N, state + weights::sW, state, cache, part, (double*)nullptr);
    else SGMCMC_LAUNCH((weights::slice_kernel<weights::kStack, false>), grid, block, 0, s, P, model_stride, K, N,
                       state + weights::sW, state, cache, part, (double*)nullptr);
    SGMCMC_LAUNCH(weights::stack_finish_kernel, dim3(1), dim3(64), 0, s, part, slices, K, N, state);
  }
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_mixture_lpd(const double* P, int64_t model_stride, int models, int64_t observations,
                                  const double* w, void* workspace, int64_t workspace_bytes, double* pointwise,
                                  double* total, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const int K = models;
  const int64_t N = observations;
  if (!w || !pointwise || !total ||
      !weights::valid_call(P, model_stride, K, N, workspace, workspace_bytes, weights::stack_bytes(K, N, false)))
    return (int)hipErrorInvalidValue;
  const int64_t slices = weights::slices_of(N);
  hipStream_t s = (hipStream_t)stream;
  SGMCMC_LAUNCH((weights::slice_kernel<weights::kMix, false>), dim3((unsigned)slices), dim3(weights::kT), 0, s, P,
                model_stride, K, N, w, (const double*)nullptr, (const double*)nullptr, (double*)workspace, pointwise);
  SGMCMC_LAUNCH(weights::mix_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, slices, K, total);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_pseudo_bma(const double* P, int64_t model_stride, int models, int64_t observations,
                                 void* workspace, int64_t workspace_bytes, double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const int K = models;
  const int64_t N = observations;
  if (!out || !weights::valid_call(P, model_stride, K, N, workspace, workspace_bytes, weights::stack_bytes(K, N, false)))
    return (int)hipErrorInvalidValue;
  const int64_t slices = weights::slices_of(N);
  hipStream_t s = (hipStream_t)stream;
  SGMCMC_LAUNCH((weights::slice_kernel<weights::kRowSum, false>), dim3((unsigned)slices), dim3(weights::kT), 0, s, P,
                model_stride, K, N, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr,
                (double*)workspace, (double*)nullptr);
  SGMCMC_LAUNCH(weights::bma_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, slices, K, out);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_bb_pseudo_bma(const double* P, int64_t model_stride, int models, int64_t observations,
                                    int64_t replicates, uint64_t seed, uint32_t noise_stream, void* workspace,
                                    int64_t workspace_bytes, double* z, double* w, double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const int K = models;
  const int64_t N = observations, B = replicates;
  if (!z || !w || !out || B < 1 ||
      !weights::valid_call(P, model_stride, K, N, workspace, workspace_bytes, weights::replicate_bytes(K, N)))
    return (int)hipErrorInvalidValue;
  const int64_t slices = weights::slices_of(N);
  // as many replicates per launch as the workspace holds, the grid's second dimension and a 2^31 grid allow
  int64_t chunk = workspace_bytes / weights::replicate_bytes(K, N);
  if (chunk > 65535) chunk = 65535;
  if (chunk > 0x7fffffffll / slices) chunk = 0x7fffffffll / slices;
  if (chunk > B) chunk = B;
  if (chunk < 1) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t count = B - b0 < chunk ? B - b0 : chunk;
    SGMCMC_LAUNCH(weights::boot_kernel, dim3((unsigned)slices, (unsigned)count), dim3(weights::kT), 0, s, P,
                  model_stride, K, N, seed, noise_stream, b0, slices, part);
    SGMCMC_LAUNCH(weights::boot_row_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, (const double*)part,
                  slices, K, N, b0, count, z, w);
  }
  SGMCMC_LAUNCH(weights::boot_total_kernel, dim3(1), dim3(weights::kT), 0, s, (const double*)z, (const double*)w, B, K,
                out);
  return (int)hipGetLastError();
}
