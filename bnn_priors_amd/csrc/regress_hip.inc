// Predictive scores of a regression posterior (evaluation side, fp64, deterministic; the reference has none of them).
// Per row n and output d the posterior predictive is the equal-weight Gaussian mixture of the E samples' Normal(mu_e,
// sigma_e); an "entry" is one (n, d), K = N D of them.  Four kernels:
//
//   pair_kernel      the pair term of the mixture's CRPS, sum_{i<j} A(mu_i - mu_j, sqrt(sigma_i^2 + sigma_j^2)).  The
//                    samples are cut into tiles of kTile; the triangle of tile pairs (I <= J) of one entry is cut into
//                    S consecutive chunks, one workgroup each (S from (E, N, D) alone: gmix_split).  A workgroup keeps
//                    tile J's (mu, sigma^2) in LDS (2 KiB), thread (i, half) owns sample i of tile I and every second
//                    j, adds its terms with Neumaier's compensation and the workgroup's 256 sums in a two-sum tree;
//                    one partial per workgroup.
//   rows_kernel      everything that is O(E) per entry: 16 entries x 16 sample slices per workgroup (a 128-byte run of
//                    the [E][K] table per load).  Pass 1: the predictive mean; pass 2: the variances and, with y, the
//                    squared error, the log density (num::lse_add1 per slice, merged on the slices' maximum), the PIT
//                    and the CRPS' first term; it then adds the entry's S pair partials in order and finishes the CRPS.
//   quantile_kernel  F(q) = p by a safeguarded secant (Illinois) inside the component-quantile hull, bisecting whenever
//                    a step fails to halve the bracket; the same 16 x 16 layout, every F a slice-wise sum.
//   pit_kernel       one workgroup per output over its ordered PIT values: the Kolmogorov-Smirnov distance to the
//                    uniform, integer counts at the levels and in the central intervals, the calibration error.
//
// Every sum runs in an order fixed by the sizes alone; counts are integers.  No atomics, no host round trip.

namespace regress {

constexpr int kTile = 128;               // samples of one LDS tile of the pair sum
constexpr int kMaxSamples = 32768;
constexpr int kTargetGroups = 2048;      // workgroups the pair sum aims at: 8 per CU
constexpr int kEntries = 16;             // entries of a rows / quantile workgroup ...
constexpr int kSlices = 16;              // ... and the slices its samples are dealt to
constexpr int kMaxQuantiles = 64;
constexpr int kMaxLevels = 1024;
constexpr int kPitThreads = 1024;
constexpr int kRootCap = 256;            // iterations of the root search, at most
static_assert(kEntries * kSlices == 256 && 2 * kTile == 256 && kMaxLevels == kPitThreads, "workgroup geometry");
static_assert(kTile == SGMCMC_GMIX_TILE && kMaxSamples == SGMCMC_GMIX_MAX_SAMPLES &&
              kMaxQuantiles == SGMCMC_GMIX_MAX_QUANTILES && kMaxLevels == SGMCMC_PIT_MAX_LEVELS, "the header's limits");

using num::comp_add;

// A(m, s) = m erf(m / (s sqrt 2)) + 2 s phi(m / s) = E|X| of X ~ Normal(m, s)
__device__ __forceinline__ double abs_moment(double m, double s) {
  const double z = m / s;
  return m * erf(z * num::kInvSqrt2) + 2.0 * s * (num::kInvSqrt2Pi * exp(-0.5 * (z * z)));
}

// Phi(z) = erfc(-z / sqrt 2) / 2: both tails keep their relative accuracy
__device__ __forceinline__ double normal_cdf(double z) { return 0.5 * erfc(-(z * num::kInvSqrt2)); }

inline int tiles_of(int E) { return (E + kTile - 1) / kTile; }

// S, the workgroups an entry's tile-pair triangle is cut into: enough for kTargetGroups over the K entries, and at most
// half the P tile pairs (a chunk of two amortises its hand-over; a diagonal pair is half a pair's work)
inline int gmix_split(int E, int64_t K) {
  const int64_t T = tiles_of(E), P = T * (T + 1) / 2;
  const int64_t want = (kTargetGroups + K - 1) / K, most = (P + 1) / 2;
  return (int)(want < most ? want : most);
}

__global__ __launch_bounds__(256) void pair_kernel(const double* __restrict__ mean, const double* __restrict__ scale,
                                                   int64_t sE, int64_t sN, int64_t sD, int E, int64_t K, int D, int S,
                                                   double* __restrict__ partial) {
  __shared__ double mu_s[kTile], var_s[kTile], red_s[256], red_c[256];
  const int t = threadIdx.x, ti = t & (kTile - 1), half = t >> 7;
  const int64_t k = blockIdx.x / (unsigned)S;
  const int c = (int)(blockIdx.x - k * S);
  const int64_t n = k / D, d = k - n * D;
  const double* __restrict__ mk = mean + k;
  const double* __restrict__ sk = scale + n * sN + d * sD;
  const int T = (E + kTile - 1) / kTile;
  const int64_t P = (int64_t)T * (T + 1) / 2;
  const int64_t p0 = c * P / S, p1 = (c + 1) * P / S;        // the chunk's tile pairs, row by row of the triangle
  int I = 0;
  int64_t rem = p0;
  while (rem >= T - I) { rem -= T - I; ++I; }
  int J = I + (int)rem;
  double sum = 0.0, comp = 0.0, mi = 0.0, vi = 0.0;
  int have = -1;
  for (int64_t p = p0; p < p1; ++p) {
    const int i = I * kTile + ti;
    if (have != I) {
      if (i < E) {
        const double sg = sk[(int64_t)i * sE];
        mi = mk[(int64_t)i * K];
        vi = sg * sg;
      }
      have = I;
    }
    const int j0 = J * kTile, cnt = min(kTile, E - j0);
    __syncthreads();
    if (t < cnt) {
      const double sg = sk[(int64_t)(j0 + t) * sE];
      mu_s[t] = mk[(int64_t)(j0 + t) * K];
      var_s[t] = sg * sg;
    }
    __syncthreads();
    if (i < E) {
      for (int jj = (I == J ? ti + 1 : 0) + half; jj < cnt; jj += 2)       // the diagonal tile: j > i only
        comp_add(sum, comp, abs_moment(mi - mu_s[jj], sqrt(vi + var_s[jj])));
    }
    if (++J == T) { ++I; J = I; }
  }
  red_s[t] = sum;
  red_c[t] = comp;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      double err;
      red_s[t] = num::two_sum(red_s[t], red_s[t + h], err);
      red_c[t] = (red_c[t] + red_c[t + h]) + err;
    }
    __syncthreads();
  }
  if (t == 0) partial[blockIdx.x] = red_s[0] + red_c[0];
}

// The sum over the 16 slices of an entry of (s + c), added in slice order with compensation: every thread of the entry
// gets the same bits.  Called by the whole workgroup.
__device__ __noinline__ double slice_sum(double* bs, double* bc, double s, double c) {
  const int t = threadIdx.x, r = t & (kEntries - 1);
  __syncthreads();
  bs[t] = s;
  bc[t] = c;
  __syncthreads();
  double S = 0.0, C = 0.0;
#pragma unroll
  for (int q = 0; q < kSlices; ++q) {
    comp_add(S, C, bs[q * kEntries + r]);
    C += bc[q * kEntries + r];
  }
  return S + C;
}

template <bool kMax>
__device__ __noinline__ double slice_extreme(double* bs, double v) {
  const int t = threadIdx.x, r = t & (kEntries - 1);
  __syncthreads();
  bs[t] = v;
  __syncthreads();
  double m = bs[r];
#pragma unroll
  for (int q = 1; q < kSlices; ++q) m = kMax ? fmax(m, bs[q * kEntries + r]) : fmin(m, bs[q * kEntries + r]);
  return m;
}

__device__ __noinline__ int slice_any(int* bi, int v) {
  const int t = threadIdx.x, r = t & (kEntries - 1);
  __syncthreads();
  bi[t] = v;
  __syncthreads();
  int any = 0;
#pragma unroll
  for (int q = 0; q < kSlices; ++q) any |= bi[q * kEntries + r];
  return any;
}

__global__ __launch_bounds__(256) void rows_kernel(const double* __restrict__ mean, const double* __restrict__ scale,
                                                   int64_t sE, int64_t sN, int64_t sD, const double* __restrict__ y,
                                                   int E, int64_t K, int D, const double* __restrict__ partial, int S,
                                                   double* __restrict__ o_mean, double* __restrict__ o_alea,
                                                   double* __restrict__ o_epi, double* __restrict__ o_var,
                                                   double* __restrict__ o_sq, double* __restrict__ o_lpd,
                                                   double* __restrict__ o_pit, double* __restrict__ o_crps) {
  __shared__ double bs[256], bc[256];
  __shared__ int bi[256];
  const int t = threadIdx.x, r = t & (kEntries - 1), q = t >> 4;
  const int64_t k_raw = (int64_t)blockIdx.x * kEntries + r;
  const bool live = k_raw < K;
  const int64_t k = live ? k_raw : 0;              // a dead lane walks entry 0 and writes nothing
  const int64_t n = k / D, d = k - n * D;
  const double* __restrict__ mk = mean + k;
  const double* __restrict__ sk = scale + n * sN + d * sD;
  const double yv = y ? y[k] : 0.0;

  double s = 0.0, c = 0.0;
  int bad = yv != yv;
#pragma unroll 1
  for (int e = q; e < E; e += kSlices) {
    const double mu = mk[(int64_t)e * K], sg = sk[(int64_t)e * sE];
    bad |= !(sg > 0.0) | (mu != mu);
    comp_add(s, c, mu);
  }
  const double mbar = slice_sum(bs, bc, s, c) / (double)E;
  bad = slice_any(bi, bad);

  double va = 0.0, va_c = 0.0, ve = 0.0, ve_c = 0.0, a1 = 0.0, a1_c = 0.0, sgs = 0.0, sgs_c = 0.0, pit = 0.0, pit_c = 0.0;
  double lm = -INFINITY, ls = 0.0;
#pragma unroll 1
  for (int e = q; e < E; e += kSlices) {
    const double mu = mk[(int64_t)e * K], sg = sk[(int64_t)e * sE];
    const double dm = mu - mbar;
    comp_add(va, va_c, sg * sg);
    comp_add(ve, ve_c, dm * dm);
    if (y) {
      const double m = yv - mu, z = m / sg;
      comp_add(a1, a1_c, abs_moment(m, sg));
      comp_add(sgs, sgs_c, sg);
      comp_add(pit, pit_c, normal_cdf(z));
      num::lse_add1(lm, ls, (-0.5 * (z * z) - log(sg)) - num::kHalfLog2Pi);
    }
  }
  const double nan = num::qnan();
  const double alea = slice_sum(bs, bc, va, va_c) / (double)E;
  const double epi = slice_sum(bs, bc, ve, ve_c) / (double)E;
  const bool writer = live && q == 0;
  if (writer) {
    o_mean[k] = bad ? nan : mbar;
    o_alea[k] = bad ? nan : alea;
    o_epi[k] = bad ? nan : epi;
    o_var[k] = bad ? nan : alea + epi;
  }
  if (!y) return;                                   // (uniform: y is a kernel argument)
  const double first = slice_sum(bs, bc, a1, a1_c);
  const double sg_sum = slice_sum(bs, bc, sgs, sgs_c);
  const double u = slice_sum(bs, bc, pit, pit_c) / (double)E;
  // the slices' log-sum-exps on their common maximum, in slice order
  const double top = slice_extreme<true>(bs, lm);
  const double part = (lm == -INFINITY || ls == 0.0) ? ls : ls * exp(lm - top);
  const double total = slice_sum(bs, bc, part, 0.0);
  const double lpd = num::lse_log_mean(top, total, E);
  // the pair partials of this entry, dealt to the slices in order
  double ps = 0.0, pc = 0.0;
  for (int j = q; j < S; j += kSlices) comp_add(ps, pc, partial[k * S + j]);
  const double pairs = slice_sum(bs, bc, ps, pc);
  if (writer) {
    const double de = yv - mbar;
    o_sq[k] = bad ? nan : de * de;
    o_lpd[k] = bad ? nan : lpd;
    o_pit[k] = bad ? nan : u;
    o_crps[k] = bad ? nan : first / (double)E - (pairs + sg_sum * num::kInvSqrtPi) / ((double)E * (double)E);
  }
}

__global__ __launch_bounds__(256) void quantile_kernel(const double* __restrict__ mean, const double* __restrict__ scale,
                                                       int64_t sE, int64_t sN, int64_t sD, int E, int64_t K, int D,
                                                       int Q, const double* __restrict__ probs,
                                                       const double* __restrict__ zs, double* __restrict__ out) {
  __shared__ double bs[256], bc[256];
  __shared__ int bi[256];
  const int t = threadIdx.x, r = t & (kEntries - 1), q = t >> 4;
  const int64_t item_raw = (int64_t)blockIdx.x * kEntries + r;      // item = level * K + entry
  const bool live = item_raw < (int64_t)Q * K;
  const int64_t item = live ? item_raw : 0;
  const int64_t lvl = item / K, k = item - lvl * K;
  const int64_t n = k / D, d = k - n * D;
  const double* __restrict__ mk = mean + k;
  const double* __restrict__ sk = scale + n * sN + d * sD;
  const double p = probs[lvl], z = zs[lvl];

  double lo = INFINITY, hi = -INFINITY;
  int bad = 0;
#pragma unroll 1
  for (int e = q; e < E; e += kSlices) {
    const double mu = mk[(int64_t)e * K], sg = sk[(int64_t)e * sE];
    bad |= !(sg > 0.0) | (mu != mu);
    const double cq = mu + sg * z;                  // this component's own p-quantile
    lo = fmin(lo, cq);
    hi = fmax(hi, cq);
  }
  lo = slice_extreme<false>(bs, lo);
  hi = slice_extreme<true>(bs, hi);
  bad = slice_any(bi, bad);

  auto cdf = [&](double x) {
    double s = 0.0, c = 0.0;
#pragma unroll 1
    for (int e = q; e < E; e += kSlices) comp_add(s, c, normal_cdf((x - mk[(int64_t)e * K]) / sk[(int64_t)e * sE]));
    return slice_sum(bs, bc, s, c) / (double)E;
  };
  // F(lo) <= p <= F(hi) in exact arithmetic; an end that already meets p (E = 1, equal components, rounding) is the root
  const double f_lo = cdf(lo), f_hi = cdf(hi);
  double r_lo = p - f_lo, r_hi = f_hi - p;          // the ends' residuals, both > 0 while the search is open
  bool done = bad || !live || !(lo < hi) || !(r_lo > 0.0) || !(r_hi > 0.0);
  if (!(lo < hi) || !(r_lo > 0.0)) { hi = lo; r_hi = r_lo = 0.0; }
  else if (!(r_hi > 0.0)) { lo = hi; r_hi = r_lo = 0.0; }
  double w_lo = r_lo, w_hi = r_hi;                  // the secant's weights: Illinois halves the one of a stuck end
  int side = 0;
  bool bisect = false;
  for (int it = 0; it < kRootCap; ++it) {
    const double mid = lo + 0.5 * (hi - lo);
    const bool open = !done && lo < mid && mid < hi;          // closed: the ends are adjacent doubles, or F(x) == p
    if (!__syncthreads_or(open)) break;
    double x = lo + (hi - lo) * (w_lo / (w_lo + w_hi));
    if (bisect || !(lo < x && x < hi)) x = mid;
    const double f = cdf(open ? x : lo);
    if (open) {
      const double width = hi - lo;
      if (f == p) {
        lo = hi = x;
        r_lo = r_hi = 0.0;
        done = true;
      } else if (f < p) {
        lo = x;
        r_lo = w_lo = p - f;
        if (side < 0) w_hi *= 0.5;
        side = -1;
      } else {
        hi = x;
        r_hi = w_hi = f - p;
        if (side > 0) w_lo *= 0.5;
        side = 1;
      }
      bisect = !bisect && (hi - lo) > 0.5 * width;            // a step that did not halve the bracket: bisect next
    }
  }
  if (live && q == 0) out[item] = bad ? num::qnan() : (r_lo <= r_hi ? lo : hi);
}

// pit: column `col` holds n values at pit[col * col_stride + i * elem_stride]; perm = sgmcmc_stable_order of the columns.
// out[col][0..2] = {ks, calibration error, has_nan}, then the n_levels counts #{u <= p_j}, then the n_central counts.
__global__ __launch_bounds__(kPitThreads) void pit_kernel(const double* __restrict__ pit, int64_t elem_stride,
                                                          int64_t col_stride, const int32_t* __restrict__ perm, int n,
                                                          const double* __restrict__ levels, int n_levels,
                                                          const double* __restrict__ central, int n_central,
                                                          double* __restrict__ out) {
  __shared__ double red[kPitThreads];
  const int t = threadIdx.x, col = blockIdx.x;
  const double* __restrict__ u = pit + (int64_t)col * col_stride;
  const int32_t* __restrict__ pc = perm + (int64_t)col * n;
  double* __restrict__ o = out + (int64_t)col * (3 + n_levels + n_central);
  auto sorted = [&](int i) { return u[(int64_t)min(max(pc[i], 0), n - 1) * elem_stride]; };
  const double last = sorted(n - 1);
  if (last != last) {                               // NaN sorts last: the column holds one
    for (int i = t; i < 3 + n_levels + n_central; i += kPitThreads) o[i] = i == 2 ? 1.0 : last;
    return;
  }
  auto count_below = [&](double v, bool inclusive) {           // #{u < v}, or #{u <= v}
    int a = 0, b = n;
    while (a < b) {
      const int mid = (a + b) >> 1;
      const double w = sorted(mid);
      if (inclusive ? w <= v : w < v) a = mid + 1; else b = mid;
    }
    return a;
  };
  double ks = 0.0;
  for (int i = t; i < n; i += kPitThreads) {
    const double v = sorted(i);
    ks = fmax(ks, fmax((double)(i + 1) / (double)n - v, v - (double)i / (double)n));
  }
  red[t] = ks;
  __syncthreads();
  for (int h = kPitThreads / 2; h > 0; h >>= 1) {
    if (t < h) red[t] = fmax(red[t], red[t + h]);
    __syncthreads();
  }
  if (t == 0) { o[0] = red[0]; o[2] = 0.0; }
  __syncthreads();
  double term = 0.0;
  if (t < n_levels) {
    const double p = levels[t];
    const int cnt = count_below(p, true);
    const double gap = (double)cnt / (double)n - p;
    o[3 + t] = (double)cnt;
    term = gap * gap;
  }
  red[t] = term;
  __syncthreads();
  for (int h = kPitThreads / 2; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) o[1] = red[0] / (double)n_levels;
  for (int i = t; i < n_central; i += kPitThreads) {
    const double cl = central[i];
    o[3 + n_levels + i] = (double)(count_below((1.0 + cl) / 2.0, true) - count_below((1.0 - cl) / 2.0, false));
  }
}

inline bool bad_sizes(int samples, int rows, int outputs) {
  return samples <= 0 || samples > kMaxSamples || rows <= 0 || outputs <= 0 ||
         (int64_t)rows * outputs > (int64_t)1 << 30;
}

}  // namespace regress

extern "C" int64_t sgmcmc_gmix_workspace_bytes(int samples, int rows, int outputs) {
  if (regress::bad_sizes(samples, rows, outputs)) return -1;
  const int64_t K = (int64_t)rows * outputs;
  return K * regress::gmix_split(samples, K) * (int64_t)sizeof(double);
}

extern "C" int sgmcmc_gmix_rows(const double* mean, const double* scale, int64_t scale_se, int64_t scale_sn,
                                int64_t scale_sd, const double* y, int samples, int rows, int outputs, void* workspace,
                                int64_t workspace_bytes, double* pred_mean, double* var_aleatoric,
                                double* var_epistemic, double* var_total, double* sq_err, double* lpd, double* pit,
                                double* crps, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const bool with = y != nullptr;
  if (!mean || !scale || !pred_mean || !var_aleatoric || !var_epistemic || !var_total || with != (sq_err != nullptr) ||
      with != (lpd != nullptr) || with != (pit != nullptr) || with != (crps != nullptr) || scale_se < 0 ||
      scale_sn < 0 || scale_sd < 0 || regress::bad_sizes(samples, rows, outputs))
    return (int)hipErrorInvalidValue;
  const int64_t K = (int64_t)rows * outputs;
  const int S = regress::gmix_split(samples, K);
  if (with) {
    if (!workspace || workspace_bytes < K * S * (int64_t)sizeof(double)) return (int)hipErrorInvalidValue;
    SGMCMC_LAUNCH(regress::pair_kernel, dim3((unsigned)(K * S)), dim3(256), 0, (hipStream_t)stream, mean, scale,
                  scale_se, scale_sn, scale_sd, samples, K, outputs, S, (double*)workspace);
  }
  SGMCMC_LAUNCH(regress::rows_kernel, dim3((unsigned)((K + regress::kEntries - 1) / regress::kEntries)), dim3(256), 0,
                (hipStream_t)stream, mean, scale, scale_se, scale_sn, scale_sd, y, samples, K, outputs,
                (const double*)workspace, S, pred_mean, var_aleatoric, var_epistemic, var_total, sq_err, lpd, pit, crps);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_gmix_quantiles(const double* mean, const double* scale, int64_t scale_se, int64_t scale_sn,
                                     int64_t scale_sd, int samples, int rows, int outputs, const double* probs,
                                     const double* z, int n_probs, double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!mean || !scale || !probs || !z || !out || scale_se < 0 || scale_sn < 0 || scale_sd < 0 || n_probs <= 0 ||
      n_probs > regress::kMaxQuantiles || regress::bad_sizes(samples, rows, outputs))
    return (int)hipErrorInvalidValue;
  const int64_t K = (int64_t)rows * outputs, items = K * n_probs;
  SGMCMC_LAUNCH(regress::quantile_kernel, dim3((unsigned)((items + regress::kEntries - 1) / regress::kEntries)),
                dim3(256), 0, (hipStream_t)stream, mean, scale, scale_se, scale_sn, scale_sd, samples, K, outputs,
                n_probs, probs, z, out);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_pit_calibration(const double* pit, int64_t elem_stride, int64_t col_stride, const int32_t* perm,
                                      int n, int ncols, const double* levels, int n_levels, const double* central,
                                      int n_central, double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!pit || !perm || !levels || !out || n <= 0 || n > calib::kMaxRows || ncols <= 0 || ncols > 65535 ||
      elem_stride <= 0 || col_stride < 0 || n_levels <= 0 || n_levels > regress::kMaxLevels || n_central < 0 ||
      n_central > regress::kMaxLevels || (n_central > 0 && !central))
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(regress::pit_kernel, dim3((unsigned)ncols), dim3(regress::kPitThreads), 0, (hipStream_t)stream, pit,
                elem_stride, col_stride, perm, n, levels, n_levels, central, n_central, out);
  return (int)hipGetLastError();
}
