// PSIS-LOO and WAIC (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024; Watanabe 2010; the
// generalised Pareto fit of Zhang and Stephens 2009) of a table ll[s][i] of S draws x N observations.
// include/sgmcmc_hip.h states the definition; this is the device path.  Lane = observation everywhere, so a draw's row
// of the table is read coalesced, and a column is only ever touched by threads of its own lane.
//
//   stats_kernel    one thread per column, two streaming passes: min / max / sum of ll, then sum exp(ll - max), the
//                   centred squares and #{x > log DBL_MIN}; the non-finite flag and the column's M
//   select_kernel   selection by counting, as rankdiag::score_kernel ranks: a thread owns kOwn consecutive draws of its
//                   column in registers and streams the column in three stretches (before, inside, after its own block),
//                   so that `less`, `equal` and `equal with a smaller draw index` are plain counts.  A draw with
//                   less >= S - M and x > log DBL_MIN is in the tail, at row S - 1 - less - before COUNTED FROM THE TOP
//                   (row 0: the largest; needs no n2), where it stores its x; every draw stores its row (or kNone) in
//                   pos[s].  The draw with less <= S - M - 1 < less + equal is the cutoff: it stores x and less + equal.
//                   S^2 N compares: the bound resource.
//   fit_kernel      one thread per column: n2, cut, ec; t_j in place of the tail's x; m + 1 passes of log1p over the
//                   column's tail (ascending j = descending row); L_j of the lane in LDS ([kMaxM][64], no exchange
//                   between lanes, hence no barrier)
//   finish_kernel   one thread per column: the smoothed, truncated tail values in place of t; then four streaming passes
//                   (max x; sum exp; lw and max (lw + ll); sum exp) and the pointwise outputs
//   totals_kernel   one workgroup: thread t adds elements t, t + 256, ... in ascending order, then a fixed tree in LDS
//
// No atomics; positions are integer counts, so no schedule changes a bit; a column's result is a function of that column
// (and its r_eff) only, whatever the grid or the chunk.

namespace psis {

constexpr int kOwn = SGMCMC_PSIS_OWN;
constexpr int kLanes = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kLanes * kWaves;
constexpr int kMaxTail = SGMCMC_PSIS_MAX_TAIL;
constexpr int kMaxM = 54;                          // 30 + floor(sqrt(544)) = 53
constexpr unsigned short kNone = 0xffff;
constexpr double kLogMin = SGMCMC_PSIS_LOG_DBL_MIN;
constexpr int kCol = 6;                            // fp64 rows of a chunk's column record
enum { cRmax, cLppd, cPwaic, cXk, cKhat, cSigma };
constexpr int kInt = 4;                            // int32 rows
enum { iM, iAbove, iLe, iFlag };
static_assert(kMaxTail < kNone && 30 + 23 < kMaxM && 23 * 23 <= kMaxTail && kMaxTail < 24 * 24, "tail limits");

// a chunk of W observations in the workspace: tail [rows][W] fp64, col [kCol][W] fp64, num [kInt][W] int32,
// pos [S][W] uint16
struct Work {
  double* tail;
  double* col;
  int* num;
  unsigned short* pos;
  int rows;
};

inline int64_t bytes_per_observation(int S, int rows) {
  return (int64_t)rows * 8 + kCol * 8 + kInt * 4 + (int64_t)S * 2;
}

inline int tail_rows(int S, bool has_r_eff) {      // an upper bound of every column's M
  const double fifth = 0.2 * (double)S, root = 3.0 * sqrt((double)S);
  const int m = (int)ceil(has_r_eff ? fifth : fmin(fifth, root));
  return m < kMaxTail ? m : kMaxTail;
}

inline Work carve(void* workspace, int64_t W, int rows) {
  Work K;
  char* p = (char*)workspace;
  K.tail = (double*)p;
  p += (int64_t)rows * W * 8;
  K.col = (double*)p;
  p += (int64_t)kCol * W * 8;
  K.num = (int*)p;
  p += (int64_t)kInt * W * 4;
  K.pos = (unsigned short*)p;
  K.rows = rows;
  return K;
}

template <typename T>
__global__ __launch_bounds__(kLanes) void stats_kernel(const T* __restrict__ tab, double lsign, int64_t stride, int S,
                                                       int64_t W, const double* __restrict__ r_eff, Work K) {
  const int64_t q = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  if (q >= W) return;
  const T* __restrict__ col = tab + q;
  bool finite = true;
  double mn = INFINITY, mx = -INFINITY, sum = 0.0;
  for (int s = 0; s < S; ++s) {
    const double v = lsign * (double)col[(int64_t)s * stride];
    finite = finite && fabs(v) < INFINITY;
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
    sum = __dadd_rn(sum, v);
  }
  const double re = r_eff ? r_eff[q] : 1.0;
  finite = finite && re > 0.0 && re < INFINITY;
  K.num[iFlag * W + q] = finite ? 0 : 1;
  if (!finite) return;
  const double rmax = -mn, mean = sum / (double)S;
  double se = 0.0, ssq = 0.0;
  int above = 0;
  for (int s = 0; s < S; ++s) {
    const double v = lsign * (double)col[(int64_t)s * stride];
    se = __dadd_rn(se, exp(__dsub_rn(v, mx)));
    const double d = __dsub_rn(v, mean);
    ssq = __dadd_rn(ssq, __dmul_rn(d, d));
    above += __dsub_rn(-v, rmax) > kLogMin;
  }
  const double m = ceil(fmin(__dmul_rn(0.2, (double)S), __dmul_rn(3.0, sqrt((double)S / re))));
  K.col[cRmax * W + q] = rmax;
  K.col[cLppd * W + q] = __dsub_rn(__dadd_rn(mx, log(se)), log((double)S));
  K.col[cPwaic * W + q] = ssq / (double)(S - 1);
  K.num[iM * W + q] = m < (double)kMaxTail ? (int)m : kMaxTail;
  K.num[iAbove * W + q] = above;
  K.num[iLe * W + q] = S;                  // until the cutoff draw says otherwise: an empty tail
  K.col[cXk * W + q] = 0.0;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void select_kernel(const T* __restrict__ tab, double lsign, int64_t stride,
                                                           int S, int64_t W, Work K) {
  const int lane = threadIdx.x % kLanes, wave = threadIdx.x / kLanes;
  const int64_t q = (int64_t)blockIdx.x * kLanes + lane;
  const int first = ((int)blockIdx.y * kWaves + wave) * kOwn;
  if (q >= W || first >= S) return;
  if (K.num[iFlag * W + q]) {
    for (int r = 0; r < kOwn && first + r < S; ++r) K.pos[(int64_t)(first + r) * W + q] = kNone;
    return;
  }
  const T* __restrict__ col = tab + q;
  const double rmax = K.col[cRmax * W + q];
  const int M = K.num[iM * W + q];
#define PSIS_X(s) __dsub_rn(-(lsign * (double)col[(int64_t)(s) * stride]), rmax)

  double own[kOwn];
  int less[kOwn], equal[kOwn], before[kOwn];
#pragma unroll
  for (int r = 0; r < kOwn; ++r) {
    own[r] = PSIS_X(min(first + r, S - 1));        // past the end: a copy of the last draw, which stores nothing
    less[r] = 0;
    equal[r] = 0;
  }
#pragma unroll 4
  for (int s = 0; s < first; ++s) {                // every equal draw here has a smaller index
    const double v = PSIS_X(s);
#pragma unroll
    for (int r = 0; r < kOwn; ++r) {
      less[r] += v < own[r];
      equal[r] += v == own[r];
    }
  }
#pragma unroll
  for (int r = 0; r < kOwn; ++r) before[r] = equal[r];
  const int stop = min(first + kOwn, S);
  for (int s = first; s < stop; ++s) {             // the own block: an equal draw counts as before if its index is smaller
    const double v = PSIS_X(s);
#pragma unroll
    for (int r = 0; r < kOwn; ++r) {
      less[r] += v < own[r];
      equal[r] += v == own[r];
      before[r] += (v == own[r]) & (s < first + r);
    }
  }
#pragma unroll 4
  for (int s = stop; s < S; ++s) {
    const double v = PSIS_X(s);
#pragma unroll
    for (int r = 0; r < kOwn; ++r) {
      less[r] += v < own[r];
      equal[r] += v == own[r];
    }
  }
#undef PSIS_X

  const int k = S - M - 1;                         // the cutoff's position, 0 <= k <= S - 2
#pragma unroll
  for (int r = 0; r < kOwn; ++r) {
    const int i = first + r;
    if (i >= S) continue;
    const int row = S - 1 - less[r] - before[r];   // from the top; in [0, M) for a tail draw
    const bool tail = less[r] >= S - M && own[r] > kLogMin && row >= 0 && row < K.rows;
    if (tail) K.tail[(int64_t)row * W + q] = own[r];
    K.pos[(int64_t)i * W + q] = tail ? (unsigned short)row : kNone;
    if (less[r] <= k && k < less[r] + equal[r]) {  // every draw that qualifies stores the same bits
      K.col[cXk * W + q] = own[r];
      K.num[iLe * W + q] = less[r] + equal[r];
    }
  }
}

__global__ __launch_bounds__(kLanes) void fit_kernel(int S, int64_t W, Work K, double* __restrict__ fit,
                                                     int* __restrict__ counts, int64_t N) {
  __shared__ double Ls[kMaxM][kLanes];
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * kLanes + lane;
  if (q >= W) return;
  const bool bad = K.num[iFlag * W + q] != 0;
  const int M = bad ? 0 : K.num[iM * W + q];
  const int n2 = bad ? 0 : min(S - K.num[iLe * W + q], K.num[iAbove * W + q]);
  const double xk = K.col[cXk * W + q];
  const double cut = bad ? NAN : (xk > kLogMin ? xk : kLogMin);
  const double ec = exp(cut);
  double khat = bad ? NAN : INFINITY, sigma = NAN;
  if (n2 > 4) {
    double* __restrict__ t = K.tail + q;           // ascending j is row n2 - 1 - j
    for (int j = 0; j < n2; ++j) {
      const int64_t at = (int64_t)(n2 - 1 - j) * W;
      t[at] = __dsub_rn(exp(t[at]), ec);
    }
    const double dn = (double)n2;
    const int m = 30 + (int)floor(sqrt(dn));
    const double dm = (double)m;
    const double inv_max = 1.0 / t[0];
    const double third = __dmul_rn(3.0, t[(int64_t)(n2 - (n2 + 2) / 4) * W]);      // ascending index (n2 + 2) / 4 - 1
    for (int j = 1; j <= m; ++j) {
      const double b = __dadd_rn(inv_max, __dsub_rn(1.0, sqrt(dm / __dsub_rn((double)j, 0.5))) / third);
      double acc = 0.0;
      for (int i = n2 - 1; i >= 0; --i) acc = __dadd_rn(acc, log1p(-__dmul_rn(b, t[(int64_t)i * W])));
      const double kap = acc / dn;
      Ls[j - 1][lane] = __dmul_rn(dn, __dsub_rn(__dsub_rn(log(-b / kap), kap), 1.0));
    }
    double bbar = 0.0;
    for (int j = 1; j <= m; ++j) {
      const double b = __dadd_rn(inv_max, __dsub_rn(1.0, sqrt(dm / __dsub_rn((double)j, 0.5))) / third);
      const double Lj = Ls[j - 1][lane];
      double den = 0.0;
      for (int l = 0; l < m; ++l) den = __dadd_rn(den, exp(__dsub_rn(Ls[l][lane], Lj)));
      bbar = __dadd_rn(bbar, __dmul_rn(b, 1.0 / den));
    }
    double acc = 0.0;
    for (int i = n2 - 1; i >= 0; --i) acc = __dadd_rn(acc, log1p(-__dmul_rn(bbar, t[(int64_t)i * W])));
    const double kap = acc / dn;
    sigma = -kap / bbar;
    khat = __dadd_rn(__dmul_rn(dn, kap), 5.0) / __dadd_rn(dn, 10.0);
  }
  K.col[cKhat * W + q] = khat;
  K.col[cSigma * W + q] = sigma;
  K.num[iLe * W + q] = n2;                         // from here on the row holds n2
  if (fit) {
    fit[q] = sigma;
    fit[N + q] = cut;
  }
  if (counts) {
    counts[q] = M;
    counts[N + q] = n2;
  }
}

template <typename T>
__global__ __launch_bounds__(kLanes) void finish_kernel(const T* __restrict__ tab, double lsign, int64_t stride, int S,
                                                        int64_t W, Work K, double* __restrict__ pointwise,
                                                        double* __restrict__ lw, int64_t N) {
  const int64_t q = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  if (q >= W) return;
  if (K.num[iFlag * W + q]) {
    for (int o = 0; o < SGMCMC_PSIS_POINTWISE; ++o) pointwise[(int64_t)o * N + q] = NAN;
    if (lw)
      for (int s = 0; s < S; ++s) lw[(int64_t)s * N + q] = NAN;
    return;
  }
  const T* __restrict__ col = tab + q;
  const unsigned short* __restrict__ pos = K.pos + q;
  double* __restrict__ t = K.tail + q;
  const double rmax = K.col[cRmax * W + q], khat = K.col[cKhat * W + q], sigma = K.col[cSigma * W + q];
  const double xk = K.col[cXk * W + q];
  const double ec = exp(xk > kLogMin ? xk : kLogMin);
  const int n2 = K.num[iLe * W + q];
  const bool smooth = fabs(khat) < INFINITY;       // hence n2 > 4 and the tail rows hold t, which is not needed any more
  if (smooth) {
    const double dn = (double)n2;
    for (int j = 0; j < n2; ++j) {
      const double l1 = log1p(-(__dadd_rn((double)j, 0.5) / dn));
      const double g = khat == 0.0 ? -__dmul_rn(sigma, l1) : __dmul_rn(sigma, expm1(-__dmul_rn(khat, l1))) / khat;
      const double v = log(__dadd_rn(g, ec));
      t[(int64_t)(n2 - 1 - j) * W] = v < 0.0 ? v : 0.0;
    }
  }
#define PSIS_X(s, ll)                                                     \
  double x;                                                               \
  {                                                                       \
    const unsigned short p_ = pos[(int64_t)(s) * W];                      \
    const double raw_ = __dsub_rn(-(ll), rmax);                           \
    x = smooth && p_ != kNone ? t[(int64_t)p_ * W] : (raw_ < 0.0 ? raw_ : 0.0); \
  }
  double mx = -INFINITY;
  for (int s = 0; s < S; ++s) {
    const double ll = lsign * (double)col[(int64_t)s * stride];
    PSIS_X(s, ll);
    mx = x > mx ? x : mx;
  }
  double se = 0.0;
  for (int s = 0; s < S; ++s) {
    const double ll = lsign * (double)col[(int64_t)s * stride];
    PSIS_X(s, ll);
    se = __dadd_rn(se, exp(__dsub_rn(x, mx)));
  }
  const double lse = __dadd_rn(mx, log(se));
  double vmx = -INFINITY;
  for (int s = 0; s < S; ++s) {
    const double ll = lsign * (double)col[(int64_t)s * stride];
    PSIS_X(s, ll);
    const double w = __dsub_rn(x, lse);
    if (lw) lw[(int64_t)s * N + q] = w;
    const double v = __dadd_rn(w, ll);
    vmx = v > vmx ? v : vmx;
  }
  double ve = 0.0;
  for (int s = 0; s < S; ++s) {
    const double ll = lsign * (double)col[(int64_t)s * stride];
    PSIS_X(s, ll);
    ve = __dadd_rn(ve, exp(__dsub_rn(__dadd_rn(__dsub_rn(x, lse), ll), vmx)));
  }
#undef PSIS_X
  const double elpd = __dadd_rn(vmx, log(ve));
  const double lppd = K.col[cLppd * W + q], pwaic = K.col[cPwaic * W + q];
  pointwise[q] = khat;
  pointwise[N + q] = elpd;
  pointwise[2 * N + q] = lppd;
  pointwise[3 * N + q] = __dsub_rn(lppd, elpd);
  pointwise[4 * N + q] = pwaic;
  pointwise[5 * N + q] = __dsub_rn(lppd, pwaic);
}

constexpr int kTot = 256;

__global__ __launch_bounds__(kTot) void totals_kernel(const double* __restrict__ pw, int64_t N, double threshold,
                                                      double* __restrict__ out) {
  __shared__ double sh[kTot];
  __shared__ double mxs[kTot];
  __shared__ int nan_seen[kTot];
  const double dN = (double)N;
  const int rows[5] = {1, 3, 2, 5, 4};             // elpd_loo, p_loo, lppd, elpd_waic, p_waic
  const int slot[5] = {0, 2, 3, 4, 6};
  double sums[5];
  for (int k = 0; k < 5; ++k) {
    const double* __restrict__ v = pw + (int64_t)rows[k] * N;
    sums[k] = num::block_sum<kTot>(N, sh, [&](int64_t i) { return v[i]; });
  }
  double se[2];
  for (int k = 0; k < 2; ++k) {                    // se of elpd_loo and of elpd_waic: two passes
    const double* __restrict__ v = pw + (int64_t)(k == 0 ? 1 : 5) * N;
    const double mean = sums[k == 0 ? 0 : 3] / dN;
    const double ssq = num::block_sum<kTot>(N, sh, [&](int64_t i) {
      const double d = __dsub_rn(v[i], mean);
      return __dmul_rn(d, d);
    });
    se[k] = sqrt(__dmul_rn(dN, ssq / __dsub_rn(dN, 1.0)));
  }
  const double bad = num::block_sum<kTot>(N, sh, [&](int64_t i) { return pw[i] > threshold ? 1.0 : 0.0; });
  double mx = -INFINITY;
  int seen = 0;
  for (int64_t i = threadIdx.x; i < N; i += kTot) {
    const double v = pw[i];
    seen |= v != v;
    mx = v > mx ? v : mx;
  }
  mxs[threadIdx.x] = mx;
  nan_seen[threadIdx.x] = seen;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < kTot; ++t) {
      mx = mxs[t] > mx ? mxs[t] : mx;
      seen |= nan_seen[t];
    }
    for (int k = 0; k < 5; ++k) out[slot[k]] = sums[k];
    out[1] = se[0];
    out[5] = se[1];
    out[7] = bad;
    out[8] = seen ? NAN : mx;
  }
}

inline bool valid_shape(int draws, int64_t observations, int64_t stride) {
  return draws >= SGMCMC_PSIS_MIN_DRAWS && draws <= SGMCMC_PSIS_MAX_DRAWS && observations >= 1 &&
         stride >= observations;
}

}  // namespace psis

extern "C" int64_t sgmcmc_psis_workspace_bytes(int draws, int64_t observations, int has_r_eff) {
  if (!psis::valid_shape(draws, observations, observations)) return -1;
  return observations * psis::bytes_per_observation(draws, psis::tail_rows(draws, has_r_eff != 0));
}

extern "C" int sgmcmc_psis_loo(const void* table, int is_f64, int is_ratio, int64_t draw_stride, int draws,
                               int64_t observations, const double* r_eff, void* workspace, int64_t workspace_bytes,
                               double* pointwise, double* fit, int32_t* counts, double* lw, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!table || !workspace || (uintptr_t)workspace % 8 || !pointwise ||
      !psis::valid_shape(draws, observations, draw_stride))
    return (int)hipErrorInvalidValue;
  const int S = draws;
  const int64_t N = observations;
  const int rows = psis::tail_rows(S, r_eff != nullptr);
  const int64_t per = psis::bytes_per_observation(S, rows);
  // all of them at once if they fit, else chunks of a multiple of 64 (whole waves)
  int64_t chunk = workspace_bytes / per;
  if (chunk < N) chunk = chunk / psis::kLanes * psis::kLanes;
  else chunk = N;
  if (chunk < 1 || (chunk + psis::kLanes - 1) / psis::kLanes > 0x7fffffffll) return (int)hipErrorInvalidValue;
  const double lsign = is_ratio ? -1.0 : 1.0;
  const size_t item = is_f64 ? 8 : 4;
  hipStream_t s = (hipStream_t)stream;
  const int per_group = psis::kOwn * psis::kWaves;
  for (int64_t q0 = 0; q0 < N; q0 += chunk) {
    const int64_t W = N - q0 < chunk ? N - q0 : chunk;
    const psis::Work K = psis::carve(workspace, W, rows);
    const dim3 cols((unsigned)((W + psis::kLanes - 1) / psis::kLanes)), one(psis::kLanes);
    const dim3 grid(cols.x, (unsigned)((S + per_group - 1) / per_group)), block(psis::kThreads);
    const void* tab = (const char*)table + (size_t)q0 * item;
    const double* re = r_eff ? r_eff + q0 : nullptr;
    double* pw = pointwise + q0;
    double* fit_q = fit ? fit + q0 : nullptr;
    int32_t* counts_q = counts ? counts + q0 : nullptr;
    double* lw_q = lw ? lw + q0 : nullptr;
    if (is_f64) {
      SGMCMC_LAUNCH(psis::stats_kernel<double>, cols, one, 0, s, (const double*)tab, lsign, draw_stride, S, W, re, K);
      SGMCMC_LAUNCH(psis::select_kernel<double>, grid, block, 0, s, (const double*)tab, lsign, draw_stride, S, W, K);
    } else {
      SGMCMC_LAUNCH(psis::stats_kernel<float>, cols, one, 0, s, (const float*)tab, lsign, draw_stride, S, W, re, K);
      SGMCMC_LAUNCH(psis::select_kernel<float>, grid, block, 0, s, (const float*)tab, lsign, draw_stride, S, W, K);
    }
    SGMCMC_LAUNCH(psis::fit_kernel, cols, one, 0, s, S, W, K, fit_q, counts_q, N);
    if (is_f64) SGMCMC_LAUNCH(psis::finish_kernel<double>, cols, one, 0, s, (const double*)tab, lsign, draw_stride, S,
                              W, K, pw, lw_q, N);
    else SGMCMC_LAUNCH(psis::finish_kernel<float>, cols, one, 0, s, (const float*)tab, lsign, draw_stride, S, W, K, pw,
                       lw_q, N);
  }
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_psis_totals(const double* pointwise, int64_t observations, double k_threshold, double* totals,
                                  void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!pointwise || !totals || observations < 1) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(psis::totals_kernel, dim3(1), dim3(psis::kTot), 0, (hipStream_t)stream, pointwise, observations,
                k_threshold, totals);
  return (int)hipGetLastError();
}
