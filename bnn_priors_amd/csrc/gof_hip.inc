// Goodness of fit of the fitted weight priors: the distribution functions of the element-wise families and, over an
// ASCENDING array of n values, the Kolmogorov-Smirnov, Cramer-von Mises and Anderson-Darling statistics and the two sides
// of a Q-Q plot (fp64, deterministic; definitions in include/sgmcmc_hip.h, restated in tests/gof_reference.py).
//
// The heart is tail(): with z = |x - loc| / scale > 0 it returns lt = log T(z), the log of the probability beyond z on ONE
// side, formed in log space (never log() of an underflowed T), the plain T and the log density in z:
//   norm     log(erfcx(z / sqrt 2) / 2) - z^2 / 2
//   laplace  log(1/2) - z
//   t        T = I_x(nu/2, 1/2) / 2, x = nu / (nu + z^2).  With y = 1 - x = z^2 / (nu + z^2), formed from z and not from x,
//            log front = log(x^(nu/2) y^(1/2) / B(nu/2, 1/2)) = nu/2 log((nu + 1) / (nu + z^2)) + 1/2 log(y (nu + 1)) + log_const:
//            num::beta_front's formula (Stirling's remainders only: num::make_beta's log_const, here with
//            num::stirling_rest) with its two logarithms taken of quantities that have one rounding each.  Where
//            num::beta_cdf would evaluate the other tail (y < 3 / (nu + 5)): T = 1/2 - front cf(1/2, nu/2; y),
//            cf = num::beta_fraction as it is; else lt = log front + log(r / 2), r the even part of the same fraction in
//            (x, y, lambda) (num::beta_fraction_even: the plain one loses 1 / y roundings where y is small).  The density
//            is front / z.
//   gennorm  T = Q(1/beta, z^beta) / 2        dgamma  T = Q(a, z) / 2
// Q(a, x) is the regularised upper incomplete gamma function: for x < a + 1 one minus the series of P (num::gamma_series),
// else the modified Lentz evaluation of its continued fraction (num::gamma_fraction), both times the prefactor
// x^a e^-x / Gamma(a), which is kept as a logarithm
//   lp = a (log1p(u) - u) + log(a / (2 pi)) / 2 - D(a),  u = (x - a) / a   (a log(x / a) - (x - a) where |u| > 1/2),
// i.e. a log x - x - lgamma(a) with Stirling's formula applied on paper, so that near x = a, where the three terms are of
// size a log a and their sum is of size 1, nothing cancels.  D(a) = lgamma(a) - ((a - 1/2) log a - a + log(2 pi) / 2) is
// num::stirling_rest: num::log_gamma's series from a >= 10 on and a recurrence below.
//
//   cdf_kernel     element-wise F, 1 - F, log F, log(1 - F) of arbitrary points for one family
//   stat_kernel    one pass over the ascending array for up to 6 (family, parameters) records: each value is loaded once
//                  and every record is evaluated on it.  A tile is kTile consecutive values, thread t takes values t,
//                  t + 256, ...; workgroup b of blocks(n) takes tiles b, b + blocks, ... in ascending order; a thread's
//                  sums are compensated (num::comp_add), a workgroup's threads meet in a fixed tree in LDS.
//   finish_kernel  one workgroup, a thread per record: the workgroups' partials in ascending order
//   ppf_kernel     model quantiles at the plotting positions (j - 1/2) / K by Newton steps on the log-tail inside a bracket
//                  (num::Bracket), and the type-7 empirical quantiles in summary::quantile_kernel's
//                  arithmetic
//
// No atomics, no allocation; tile and grid are functions of n alone, so every sum runs in an order fixed by n.

namespace gof {

constexpr int kMaxRecords = SGMCMC_GOF_MAX_RECORDS;
constexpr int kMaxQuantiles = SGMCMC_GOF_MAX_QUANTILES;
constexpr int kThreads = 256;
constexpr int kTile = SGMCMC_GOF_TILE;
constexpr int kPer = kTile / kThreads;                 // values of a tile per thread
constexpr int kMaxBlocks = SGMCMC_GOF_MAX_BLOCKS;
constexpr int kPart = SGMCMC_GOF_PART;                 // doubles of one record's partial
constexpr int kOut = SGMCMC_GOF_OUT;
constexpr int kStride = (kMaxRecords + 1) * kPart;     // doubles of one workgroup's partials; [kMaxRecords * kPart]: bad
constexpr int64_t kMaxN = 0x7fffffffll;
constexpr int kTerms = 20000;                          // of the gamma series and of its continued fraction, at most
constexpr int kRootSteps = 200;
static_assert(kTile % kThreads == 0 && (kThreads & (kThreads - 1)) == 0, "tile");
static_assert(kPart == 8 && kOut == 8, "record layouts");

enum { kUniform = SGMCMC_GOF_UNIFORM, kNorm = SGMCMC_GOF_NORM, kLaplace = SGMCMC_GOF_LAPLACE, kT = SGMCMC_GOF_T,
       kGennorm = SGMCMC_GOF_GENNORM, kDgamma = SGMCMC_GOF_DGAMMA };
// a partial: D+, its index, D-, its index, the Cramer-von Mises sum and its compensation, the Anderson-Darling sum and its
enum { kDp = 0, kIp = 1, kDm = 2, kIm = 3, kSw = 4, kCw = 5, kSa = 6, kCa = 7 };

typedef sgmcmc_gof_record Rec;
struct Recs {
  Rec r[kMaxRecords];
  int count;
};

struct Fam {                // a record and what does not depend on x
  int family;
  double shape, loc, scale;
  double a;                 // of Q(a, .): 1 / beta, a
  double c;                 // log(a / (2 pi)) / 2 - D(a)
  double lnorm;             // the density's log constant
  double log_const;         // t: num::Beta's
};

inline bool finite_host(double v) { return v - v == 0.0; }

inline bool valid(const Rec& r) {
  if (!finite_host(r.loc) || !finite_host(r.scale) || !(r.scale > 0.0)) return false;
  switch (r.family) {
    case kUniform: case kNorm: case kLaplace: return true;
    case kT: return r.shape >= SGMCMC_GOF_DF_MIN && r.shape <= SGMCMC_GOF_DF_MAX;
    case kGennorm: return r.shape >= SGMCMC_GOF_BETA_MIN && r.shape <= SGMCMC_GOF_BETA_MAX;
    case kDgamma: return r.shape >= SGMCMC_GOF_A_MIN && r.shape <= SGMCMC_GOF_A_MAX;
    default: return false;
  }
}

inline bool make_recs(const Rec* records, int count, Recs* R) {
  if (!records || count < 1 || count > kMaxRecords) return false;
  for (int f = 0; f < kMaxRecords; ++f) {
    R->r[f] = records[f < count ? f : 0];
    if (!valid(R->r[f])) return false;
  }
  R->count = count;
  return true;
}

inline int blocks(int64_t n) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  return (int)(tiles < kMaxBlocks ? tiles : kMaxBlocks);
}

__device__ Fam prepare(const Rec& r) {
  Fam F;
  F.family = r.family;
  F.shape = r.shape;
  F.loc = r.loc;
  F.scale = r.scale;
  F.a = F.c = F.lnorm = F.log_const = 0.0;
  if (r.family == kT) {
    // num::make_beta's log_const, log(a b / (2 pi T)) / 2 + D(T) - D(a) - D(b) at a = nu / 2, b = 1 / 2, T = a + b
    const double a = 0.5 * r.shape, total = a + 0.5;
    F.log_const = 0.5 * log(0.5 * a / (num::kTwoPi * total)) + num::stirling_rest(total) - num::stirling_rest(a) -
                  num::stirling_rest(0.5);
  } else if (r.family == kGennorm || r.family == kDgamma) {
    F.a = r.family == kGennorm ? 1.0 / r.shape : r.shape;
    F.c = 0.5 * log(F.a / num::kTwoPi) - num::stirling_rest(F.a);
    F.lnorm = (r.family == kGennorm ? log(r.shape) : 0.0) + num::kLogHalf - num::log_gamma(F.a);
  }
  return F;
}

// log Q(a, x) and Q(a, x), x > 0; c = log(a / (2 pi)) / 2 - D(a)
__device__ void upper_gamma(double a, double x, double c, double* log_q, double* q) {
  const double excess = x - a, u = excess / a;
  const double lp = (fabs(u) <= 0.5 ? a * num::log1p_minus(u) : a * log(x / a) - excess) + c;
  if (x < a + 1.0) {                                  // P = e^lp sum_k x^k / (a (a + 1) .. (a + k))
    const double p = fmin(exp(lp) * num::gamma_series(a, x, kTerms), 1.0);
    *q = 1.0 - p;
    *log_q = log1p(-p);
    return;
  }
  const double h = num::gamma_fraction(a, x, kTerms);
  *log_q = lp + log(h);
  *q = exp(lp) * h;
}

struct Tail {
  double lt, T, lpdf;       // log T(z), T(z), the log density of z (one side carries half the mass)
};

__device__ Tail tail(const Fam& F, double z) {              // 0 < z < inf
  Tail r;
  switch (F.family) {
    case kNorm: {
      const double h = 0.5 * (z * z), e = 0.5 * erfcx(z * num::kInvSqrt2);
      r.lt = log(e) - h;
      r.T = e * exp(-h);
      r.lpdf = -h - num::kHalfLog2Pi;
      break;
    }
    case kLaplace:
      r.lt = num::kLogHalf - z;
      r.T = 0.5 * exp(-z);
      r.lpdf = r.lt;
      break;
    case kT: {
      const double nu = F.shape, z2 = z * z, den = nu + z2, x = nu / den, y = z2 / den;
      const double rr = (1.0 - z2) / den;                   // (nu + 1) / den - 1
      const double l1 = fabs(rr) <= 0.5 ? log1p(rr) : log((nu + 1.0) / den);
      const double lfront = 0.5 * nu * l1 + 0.5 * log(y * (nu + 1.0)) + F.log_const;
      if (y < 3.0 / (nu + 5.0)) {                           // x >= (a + 1) / (a + b + 2): the other tail
        r.T = 0.5 - exp(lfront) * num::beta_fraction(0.5, 0.5 * nu, y);
        r.lt = log(r.T);
      } else {
        const double cf = 0.5 * num::beta_fraction_even(0.5 * nu, 0.5, x, y, nu * (z2 - 1.0) / (2.0 * den));
        r.T = exp(lfront) * cf;
        r.lt = lfront + log(cf);
      }
      r.lpdf = lfront - log(z);
      break;
    }
    case kGennorm: {
      const double w = pow(z, F.shape);
      double lq, q;
      if (!(w < INFINITY)) lq = -INFINITY, q = 0.0;
      else if (w > 0.0) upper_gamma(F.a, w, F.c, &lq, &q);
      else lq = 0.0, q = 1.0;
      r.lt = lq + num::kLogHalf;
      r.T = 0.5 * q;
      r.lpdf = F.lnorm - w;
      break;
    }
    default: {                                              // kDgamma
      double lq, q;
      upper_gamma(F.a, z, F.c, &lq, &q);
      r.lt = lq + num::kLogHalf;
      r.T = 0.5 * q;
      r.lpdf = (F.a - 1.0) * log(z) - z + F.lnorm;
      break;
    }
  }
  return r;
}

struct Probs {
  double F, S, lF, lS;      // F, 1 - F and their logarithms
};

__device__ Probs probs(const Fam& F, double x) {
  Probs p;
  if (x != x) {
    p.F = p.S = p.lF = p.lS = x;
    return p;
  }
  if (F.family == kUniform) {
    const double u = fmin(fmax((x - F.loc) / F.scale, 0.0), 1.0);
    p.F = u;
    p.S = 1.0 - u;
    p.lF = log(u);
    p.lS = log1p(-u);
    return p;
  }
  const double d = x - F.loc, z = fabs(d) / F.scale;
  if (z == 0.0) {                                           // exactly one half in every symmetric family
    p.F = p.S = 0.5;
    p.lF = p.lS = num::kLogHalf;
    return p;
  }
  Tail t;
  if (z < 1e150) t = tail(F, z);                            // (beyond it z^2 overflows; every tail is 0 long before)
  else t.lt = -INFINITY, t.T = 0.0, t.lpdf = -INFINITY;
  const double big = 1.0 - t.T, lbig = log1p(-t.T);
  if (d > 0.0) {
    p.F = big; p.S = t.T; p.lF = lbig; p.lS = t.lt;
  } else {
    p.F = t.T; p.S = big; p.lF = t.lt; p.lS = lbig;
  }
  return p;
}

// the z >= 0 with log T(z) = target <= log(1/2): Newton steps on the log-tail (d lt / dz = -pdf / T) by num::Bracket,
// without an upper end at first
__device__ double tail_inverse(const Fam& F, double target) {
  num::Bracket br = {0.0, INFINITY};
  double z = 1.0;
  for (int it = 0; it < kRootSteps; ++it) {
    const Tail t = tail(F, z);
    const double g = t.lt - target;
    if (g == 0.0) return z;
    if (g > 0.0) br.lo = z;
    else br.hi = z;
    if (!br.advance(z, z + g * exp(t.lt - t.lpdf))) break;
  }
  return z;
}

__device__ double quantile(const Fam& F, double p) {
  if (F.family == kUniform) return F.loc + F.scale * p;
  if (p == 0.5) return F.loc;
  const double z = tail_inverse(F, log(p < 0.5 ? p : 1.0 - p));
  return p < 0.5 ? F.loc - F.scale * z : F.loc + F.scale * z;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void cdf_kernel(const T* __restrict__ x, int64_t m, Rec rec,
                                                       double* __restrict__ out) {
  __shared__ Fam fam;
  if (threadIdx.x == 0) fam = prepare(rec);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const Probs p = probs(fam, (double)x[i]);
  out[i] = p.F;
  out[m + i] = p.S;
  out[2 * m + i] = p.lF;
  out[3 * m + i] = p.lS;
}

// the larger value; of equal values the smaller index
__device__ __forceinline__ void take_max(double& v, double& at, double ov, double oat) {
  if (ov > v || (ov == v && oat < at)) {
    v = ov;
    at = oat;
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void stat_kernel(const T* __restrict__ x, int64_t n, Recs R,
                                                        double* __restrict__ part) {
  __shared__ Fam fam[kMaxRecords];
  __shared__ double red[kPart][kThreads];
  __shared__ long long sbad[kThreads];
  const int t = threadIdx.x;
  if (t < R.count) fam[t] = prepare(R.r[t]);
  __syncthreads();
  double acc[kMaxRecords][kPart];
#pragma unroll
  for (int f = 0; f < kMaxRecords; ++f) {
    acc[f][kDp] = acc[f][kDm] = -INFINITY;
    acc[f][kIp] = acc[f][kIm] = INFINITY;
    acc[f][kSw] = acc[f][kCw] = acc[f][kSa] = acc[f][kCa] = 0.0;
  }
  long long bad = 0;
  const int64_t tiles = (n + kTile - 1) / kTile;
  const double nd = (double)n;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (int j = 0; j < kPer; ++j) {
      const int64_t idx = tile * kTile + (int64_t)j * kThreads + t;
      if (idx >= n) break;
      const double v = (double)x[idx];
      if (!num::is_finite(v)) {
        ++bad;
        continue;
      }
      const double i = (double)(idx + 1), odd = 2.0 * i - 1.0;         // exact: i <= 2^31
      const double above = i / nd, below = (i - 1.0) / nd, centre = odd / (2.0 * nd), rest = 2.0 * (nd - i) + 1.0;
#pragma unroll
      for (int f = 0; f < kMaxRecords; ++f) {
        if (f < R.count) {
          const Probs p = probs(fam[f], v);
          const double dp = above - p.F, dm = p.F - below, e = p.F - centre;
          if (dp > acc[f][kDp]) acc[f][kDp] = dp, acc[f][kIp] = i;      // strict: the smallest index of a thread's walk
          if (dm > acc[f][kDm]) acc[f][kDm] = dm, acc[f][kIm] = i;
          num::comp_add(acc[f][kSw], acc[f][kCw], e * e);
          num::comp_add(acc[f][kSa], acc[f][kCa], odd * p.lF + rest * p.lS);
        }
      }
    }
  }
  sbad[t] = bad;
#pragma unroll
  for (int f = 0; f < kMaxRecords; ++f) {
    if (f < R.count) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kPart; ++k) red[k][t] = acc[f][k];
      for (int s = kThreads / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) {
          const int o = t + s;
          take_max(red[kDp][t], red[kIp][t], red[kDp][o], red[kIp][o]);
          take_max(red[kDm][t], red[kIm][t], red[kDm][o], red[kIm][o]);
          num::comp_add(red[kSw][t], red[kCw][t], red[kSw][o]);
          red[kCw][t] += red[kCw][o];
          num::comp_add(red[kSa][t], red[kCa][t], red[kSa][o]);
          red[kCa][t] += red[kCa][o];
          if (f == 0) sbad[t] += sbad[o];
        }
      }
      __syncthreads();
      if (t < kPart) part[(int64_t)blockIdx.x * kStride + f * kPart + t] = red[t][0];
    }
  }
  if (t == 0) part[(int64_t)blockIdx.x * kStride + kMaxRecords * kPart] = (double)sbad[0];
}

// a compensated sum's value; an infinite sum (log 0 of a point outside the support) stays infinite
__device__ __forceinline__ double comp_value(double s, double c) { return num::is_finite(s) ? s + c : s; }

// out [count][kOut]: D, D+, D-, the 1-based index of the supremum, x there, W^2, A^2, the number of non-finite inputs
template <typename T>
__global__ __launch_bounds__(64) void finish_kernel(const T* __restrict__ x, int64_t n, int count, int nblocks,
                                                    const double* __restrict__ part, double* __restrict__ out) {
  const int f = threadIdx.x;
  if (f >= count) return;
  double dp = -INFINITY, ip = INFINITY, dm = -INFINITY, im = INFINITY, sw = 0.0, cw = 0.0, sa = 0.0, ca = 0.0;
  double bad = 0.0;
  for (int b = 0; b < nblocks; ++b) {
    const double* __restrict__ p = part + (int64_t)b * kStride + f * kPart;
    take_max(dp, ip, p[kDp], p[kIp]);
    take_max(dm, im, p[kDm], p[kIm]);
    num::comp_add(sw, cw, p[kSw]);
    cw += p[kCw];
    num::comp_add(sa, ca, p[kSa]);
    ca += p[kCa];
    bad += part[(int64_t)b * kStride + kMaxRecords * kPart];
  }
  const double nd = (double)n, at = dp >= dm ? ip : im;
  double* __restrict__ o = out + f * kOut;
  o[0] = fmax(dp, dm);
  o[1] = dp;
  o[2] = dm;
  o[3] = at;
  o[4] = at >= 1.0 && at <= nd ? (double)x[(int64_t)at - 1] : NAN;
  o[5] = 1.0 / (12.0 * nd) + comp_value(sw, cw);
  o[6] = -nd - comp_value(sa, ca) / nd;
  o[7] = bad;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void ppf_kernel(const T* __restrict__ x, int64_t n, Recs R, int K,
                                                       double* __restrict__ model, double* __restrict__ empirical) {
  __shared__ Fam fam[kMaxRecords];
  if (threadIdx.x < R.count) fam[threadIdx.x] = prepare(R.r[threadIdx.x]);
  __syncthreads();
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= R.count * K) return;
  const int f = idx / K, j = idx - f * K;
  const double p = (double)(2 * j + 1) / (double)(2 * K);               // (j + 1 - 1/2) / K
  if (f == 0) {
    // numpy's linear rule in summary::quantile_kernel's arithmetic, every operation rounded once
    const double pos = __dmul_rn((double)(n - 1), p), fl = floor(pos), frac = __dsub_rn(pos, fl);
    const int64_t lo = (int64_t)fl, hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    const double a = (double)x[lo], b = (double)x[hi], d = __dsub_rn(b, a);
    empirical[j] = frac >= 0.5 ? __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, frac))) : __dadd_rn(a, __dmul_rn(d, frac));
  }
  model[idx] = quantile(fam[f], p);
}

}  // namespace gof

extern "C" int64_t sgmcmc_gof_workspace_doubles(int64_t n) {
  if (n < 1 || n > gof::kMaxN) return -1;
  return (int64_t)gof::blocks(n) * gof::kStride;
}

extern "C" int sgmcmc_gof_cdf(const void* x, int is_f64, int64_t m, const sgmcmc_gof_record* record, double* out,
                              void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  gof::Recs R;
  if (!x || !out || m < 1 || m > gof::kMaxN || !gof::make_recs(record, 1, &R)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((m + gof::kThreads - 1) / gof::kThreads)), block(gof::kThreads);
  if (is_f64) SGMCMC_LAUNCH(gof::cdf_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x, m, R.r[0], out);
  else SGMCMC_LAUNCH(gof::cdf_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, m, R.r[0], out);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_gof_statistics(const void* sorted, int is_f64, int64_t n, const sgmcmc_gof_record* records,
                                     int count, double* workspace, double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  gof::Recs R;
  if (!sorted || !workspace || !out || n < 1 || n > gof::kMaxN || !gof::make_recs(records, count, &R))
    return (int)hipErrorInvalidValue;
  const int nb = gof::blocks(n);
  const dim3 grid((unsigned)nb), block(gof::kThreads);
  if (is_f64) {
    SGMCMC_LAUNCH(gof::stat_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)sorted, n, R, workspace);
    SGMCMC_LAUNCH(gof::finish_kernel<double>, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)sorted, n, count,
                  nb, (const double*)workspace, out);
  } else {
    SGMCMC_LAUNCH(gof::stat_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)sorted, n, R, workspace);
    SGMCMC_LAUNCH(gof::finish_kernel<float>, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)sorted, n, count,
                  nb, (const double*)workspace, out);
  }
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_gof_ppf(const void* sorted, int is_f64, int64_t n, const sgmcmc_gof_record* records, int count,
                              int K, double* model, double* empirical, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  gof::Recs R;
  if (!sorted || !model || !empirical || n < 1 || n > gof::kMaxN || K < 1 || K > gof::kMaxQuantiles ||
      !gof::make_recs(records, count, &R))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((count * K + gof::kThreads - 1) / gof::kThreads)), block(gof::kThreads);
  if (is_f64) SGMCMC_LAUNCH(gof::ppf_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)sorted, n, R, K,
                            model, empirical);
  else SGMCMC_LAUNCH(gof::ppf_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)sorted, n, R, K, model,
                     empirical);
  return (int)hipGetLastError();
}
