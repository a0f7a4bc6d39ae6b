// Sampler temperature diagnostics: does a chain sample at the temperature it claims?  A parameter tensor with d elements
// has kinetic temperature T^/T ~ chi^2_d / d, so everything here is the regularised incomplete gamma function at
// a = d / 2, d an integer in [1, 2^31 - 1], at the point x = a r, r = T^/T (fp64, deterministic; definitions in
// include/sgmcmc_hip.h, restated at 50 digits in tests/temperature_reference.py).
//
// tails(a, r): log P(a, a r), log Q(a, a r), P, Q and the prefactor's logarithm.  ONE of the two tails is evaluated, in log
// space, by the method of its region, and the other derived from it (1 - small, log1p(-small)); the evaluated one is the
// small one except in the band a <= x < a + 1 (below).  With u = r - 1 (exact for 1/2 <= r <= 2: the point is never formed
// as x - a) and l = log1p(u) - u (num::log1p_minus, no cancellation near r = 1):
//   uniform   a >= kTemmeA = 100 and |u| <= kTemmeU = 0.3: Temme's uniform expansion (SIAM J. Math. Anal. 10 (1979); DLMF
//             8.12.3-10; the form DiDonato & Morris use in TOMS 654),
//                 Q = erfc(y) / 2 + S,  P = erfc(-y) / 2 - S,  S = e^(-h) / sqrt(2 pi a) sum_k c_k(eta) a^-k,
//                 h = -a l = a eta^2 / 2,  y = sqrt(h),  eta = sign(u) sqrt(-2 l),
//             as  small = e^(-h) [erfcx(y) / 2 +- sum / sqrt(2 pi a)],  log small = -h + log[...]: O(1) work at every a, and
//             finite far beyond where e^(-h) underflows.  c_0 .. c_8 are kept as their power series in eta, generated as
//             exact rationals from  mu mu' = eta (1 + mu),  c_0 = 1 / mu - 1 / eta,  c_k = c_(k-1)' / eta + gamma_k / mu
//             (mu = u as a series in eta; gamma_k = -c_(k-1)'(0), Stirling's coefficients) and cut where the rest is below
//             3e-19 * 100^k at |eta| = 0.34 (eta(-0.3) = -0.337, eta(0.3) = 0.274); the first term left out, c_9 a^-9, is
//             below 6e-22 at a = 100.
//   series    elsewhere, x < a + 1:  P = e^lp sum_k x^k / (a (a + 1) .. (a + k))      (num::gamma_series and
//   fraction  elsewhere, x >= a + 1: Q = e^lp * the modified Lentz fraction            num::gamma_fraction)
//             lp = a l + log(a / (2 pi)) / 2 - D(a)   (a log r - a u where |u| > 1/2), D = num::stirling_rest.
//             Both need O(sqrt a) terms near x = a; outside the uniform region that is at most 8.5 sqrt(100) terms for
//             a < 100 and about 37 / 0.3 terms for |u| > 0.3 (measured: at most 99 at a = 1e9, 58 at a = 1e3), so kTerms
//             caps a loop that has ended long before.
//   In the band a <= x < a + 1 the fraction is NOT used although Q is the smaller tail there: at half-integer a its early
//   partial denominators change sign, and it was measured 33 eps off at a = 1/2, 21 eps at a = 3/2 (10 eps at a = 5/2);
//   the series' P <= 0.92 there, Q = 1 - P >= 0.083 costs at most a factor 11, measured 9.9 eps at a = 1/2, 7 eps at
//   a = 1, below 6.3 eps for a >= 3/2.
// Measured distance from the 50-digit value, |lt - exact| / max(1, |exact|) in units of eps = 2^-52, of the same
// arithmetic in fp64 on the host, x = a (1 + s / sqrt a), s = -8 .. 8:
//   a = 99.5 (series / fraction) 1.45      a = 100, 100.5 (uniform inside |s| <= 3) 1.10, 1.11
//   u = +-0.3 at a = 1e2, 1e3: uniform side 0.53, 0.54; series / fraction side 0.21, 0.51; at a = 1e6, 1e9 the two sides
//   agree to 0.3 eps of each other.  d = 1 .. 80 and 200 .. 1999 (all by series / fraction): worst 6.2 (d = 6, s = 0.3);
//   d = 2e4 .. 2^31 - 1 (uniform): worst 1.6.  The figures of the device are in tests/test_temperature.py.
//
//   tails_kernel     element-wise, one thread per (step, tensor): r = est / temperature, the four values above
//   quantile_kernel  one thread per (tensor, entry): the r with log tail(a, r) = t by Newton steps on the log-tail in r
//                    (d log P / dr = e^(lp - log r - log P)) from the Wilson-Hilferty point, inside a bracket that every
//                    evaluation narrows, kRootSteps at most (num::Bracket).  The iterate IS the returned
//                    r = x / a and the tail is evaluated at u = r - 1, so the bound carries one rounding.
//   steps_kernel     one thread per step, the tensors in ascending order: the number of tensors with lower <= r <= upper
//                    per level, Cochran's weighted mean and standard error (compensated sums, num::comp_add), and the
//                    per-tensor coverage over all steps as INTEGER counts (a wave's ballot, gathered per workgroup in LDS,
//                    one global integer atomic per workgroup, tensor and level: exact, hence independent of the order)
//   ewma_kernel      y_0 = x_0, y_t = (1 - alpha) x_t + alpha y_(t-1) as a scan of the affine maps y -> A y + B: one
//                    workgroup per row, thread t owns the ceil(S / 256) consecutive steps from t ceil(S / 256) on,
//                    composes them in order, the 256 composites meet in a Hillis-Steele scan in LDS, and the thread
//                    replays its steps from the carry.  An infinite value stays infinite in what follows it, as in
//                    the step-by-step recurrence, also where alpha^n has underflowed.  No floating-point atomics anywhere.

namespace temper {

constexpr int kThreads = 256;
constexpr int kScan = SGMCMC_TEMPER_SCAN;
constexpr int kMaxLevels = SGMCMC_TEMPER_MAX_LEVELS;
constexpr int64_t kMaxN = 0x7fffffffll;
constexpr int kTerms = 2000;                           // of the series and of the fraction, at most
constexpr int kRootSteps = 100;
constexpr int kStepBlocks = 256, kLdsCounts = 4096;     // of steps_kernel: workgroups at most; counts kept in LDS
constexpr double kTemmeA = SGMCMC_TEMPER_UNIFORM_A, kTemmeU = SGMCMC_TEMPER_UNIFORM_U;
static_assert(kScan == kThreads && (kScan & (kScan - 1)) == 0, "scan");

constexpr int kOrders = 9;
__device__ const double kTemme[86] = {
    // c_0
    -0.3333333333333333, 0.08333333333333333, -0.014814814814814815, 0.0011574074074074073, 0.0003527336860670194,
    -0.0001787551440329218, 3.919263178522438e-05, -2.185448510679992e-06, -1.85406221071516e-06,
    8.296711340953087e-07, -1.7665952736826078e-07, 6.707853543401498e-09, 1.0261809784240309e-08,
    -4.382036018453353e-09, 9.14769958223679e-10, -2.5514193994946248e-11, -5.830772132550426e-11,
    // c_1
    -0.001851851851851852, -0.003472222222222222, 0.0026455026455026454, -0.0009902263374485596,
    0.00020576131687242798, -4.018775720164609e-07, -1.8098550334489977e-05, 7.64916091608111e-06,
    -1.6120900894563446e-06, 4.647127802807434e-09, 1.378633446915721e-07, -5.752545603517705e-08,
    1.1951628599778148e-08, -1.7543241719747647e-11, -1.0091543710600413e-09, 4.162792991842583e-10,
    // c_2
    0.004133597883597883, -0.0026813271604938273, 0.0007716049382716049, 2.0093878600823047e-06,
    -0.0001073665322636516, 5.2923448829120125e-05, -1.2760635188618728e-05, 3.423578734096138e-08,
    1.3721957309062934e-06, -6.298992138380055e-07, 1.4280614206064242e-07, -2.0477098421990866e-10,
    -1.409252991086752e-08, 6.228974084922022e-09,
    // c_3
    0.0006494341563786008, 0.00022947209362139917, -0.0004691894943952557, 0.00026772063206283885,
    -7.561801671883977e-05, -2.396505113867297e-07, 1.1082654115347302e-05, -5.6749528269915965e-06,
    1.4230900732435883e-06, -2.7861080291528143e-11, -1.6958404091930278e-07, 8.099464905388083e-08,
    // c_4
    -0.0008618882909167117, 0.0007840392217200666, -0.0002990724803031902, -1.4638452578843418e-06,
    6.641498215465122e-05, -3.968365047179435e-05, 1.1375726970678419e-05, 2.507497226237533e-10,
    -1.6954149536558305e-06, 8.907507532205309e-07,
    // c_5
    -0.00033679855336635813, -6.972813758365857e-05, 0.0002772753244959392, -0.00019932570516188847,
    6.797780477937208e-05, 1.419062920643967e-07, -1.3594048189768693e-05, 8.018470256334202e-06,
    // c_6
    0.0005313079364639922, -0.0005921664373536939, 0.0002708782096718045, 7.902353232660328e-07, -8.153969367561969e-05,
    // c_7
    0.00034436760689237765, 5.171790908260592e-05, -0.00033493161081142234,
    // c_8
    -0.0006526239185953094};

struct Tails {
  double lp, lq, p, q;      // log P, log Q, P, Q
  double front;             // log(x^a e^-x / Gamma(a)): the density of r is e^front / r
};

// sum_k c_k(eta) a^-k, Horner in eta inside Horner in 1 / a
__device__ double temme_sum(double eta, double a) {
  constexpr int kDegree[kOrders] = {16, 15, 13, 11, 9, 7, 4, 2, 0};
  constexpr int kFirst[kOrders] = {0, 17, 33, 47, 59, 69, 77, 82, 85};
  static_assert(kFirst[kOrders - 1] + kDegree[kOrders - 1] + 1 == 86, "table");
  const double ia = 1.0 / a;
  double sum = 0.0;
#pragma unroll
  for (int k = kOrders - 1; k >= 0; --k) {
    double ck = 0.0;
#pragma unroll
    for (int j = kDegree[k]; j >= 0; --j) ck = ck * eta + kTemme[kFirst[k] + j];
    sum = sum * ia + ck;
  }
  return sum;
}

__device__ Tails tails(double a, double r) {
  Tails t;
  if (r != r) {
    t.lp = t.lq = t.p = t.q = t.front = r;
    return t;
  }
  if (!(r > 0.0)) {
    t.lp = -INFINITY, t.p = 0.0, t.lq = 0.0, t.q = 1.0, t.front = -INFINITY;
    return t;
  }
  const double x = a * r;
  if (!(x < INFINITY)) {
    t.lp = 0.0, t.p = 1.0, t.lq = -INFINITY, t.q = 0.0, t.front = -INFINITY;
    return t;
  }
  const double c = 0.5 * log(a / num::kTwoPi) - num::stirling_rest(a);
  const double u = r - 1.0;
  const bool near = fabs(u) <= 0.5;
  const double l = near ? num::log1p_minus(u) : 0.0;
  t.front = (near ? a * l : a * log(r) - a * u) + c;
  double small, lsmall;
  bool upper;
  if (a >= kTemmeA && fabs(u) <= kTemmeU) {
    const double h = -(a * l), y = sqrt(h);
    double eta = sqrt(-2.0 * l);
    if (u < 0.0) eta = -eta;
    const double s = temme_sum(eta, a) / sqrt(num::kTwoPi * a);
    upper = u >= 0.0;
    const double w = 0.5 * erfcx(y) + (upper ? s : -s);
    lsmall = log(w) - h;
    small = w * exp(-h);
  } else if (x < a + 1.0) {
    const double sum = num::gamma_series(a, x, kTerms);
    upper = false;
    lsmall = t.front + log(sum);
    small = exp(t.front) * sum;
  } else {
    const double h = num::gamma_fraction(a, x, kTerms);
    upper = true;
    lsmall = t.front + log(h);
    small = exp(t.front) * h;
  }
  if (!(small < 1.0)) small = 1.0, lsmall = 0.0;        // (a rounding above 1 where the other tail is below eps)
  const double other = 1.0 - small, lother = log1p(-small);
  if (upper) t.lq = lsmall, t.q = small, t.lp = lother, t.p = other;
  else t.lp = lsmall, t.p = small, t.lq = lother, t.q = other;
  return t;
}

// the r = x / a with log Q(a, a r) = target (upper) or log P(a, a r) = target; target <= 0
__device__ double tail_inverse(double a, double target, bool upper) {
  if (target != target) return target;
  if (target >= 0.0) return upper ? 0.0 : INFINITY;
  if (target == -INFINITY) return upper ? INFINITY : 0.0;
  // Wilson-Hilferty: (chi^2_d / d)^(1/3) is nearly normal with mean 1 - 2 / (9 d) and variance 2 / (9 d), d = 2 a
  double z = target > -700.0 ? normcdfinv(exp(target)) : -sqrt(-2.0 * target);
  if (upper) z = -z;
  const double w = 1.0 - 1.0 / (9.0 * a) + z / (3.0 * sqrt(a));
  double r = w * w * w;
  if (!(w > 0.0 && r > 0.0 && r < INFINITY)) {
    r = upper ? 1.0 : exp((target + lgamma(a + 1.0)) / a) / a;       // P ~ x^a / Gamma(a + 1) at small x
    if (!(r > 0.0)) r = 1e-300;
  }
  num::Bracket br = {0.0, INFINITY};
  for (int it = 0; it < kRootSteps; ++it) {
    const Tails t = tails(a, r);
    const double lt = upper ? t.lq : t.lp, g = lt - target;
    if (g == 0.0) return r;
    if ((g > 0.0) != upper) br.hi = r;                    // P rises with r, Q falls
    else br.lo = r;
    const double step = g * exp(lt - (t.front - log(r)));
    if (!br.advance(r, upper ? r + step : r - step)) break;
  }
  return r;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void tails_kernel(const T* __restrict__ est, int64_t S, int K, int64_t stride_s,
                                                         int64_t stride_k, const double* __restrict__ temperature,
                                                         int64_t temp_stride, const int64_t* __restrict__ sizes,
                                                         double* __restrict__ out) {
  const int64_t m = S * K, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const int64_t s = i / K;
  const int k = (int)(i - s * K);
  double r = (double)est[s * stride_s + k * stride_k];
  if (temperature) r = r / temperature[s * temp_stride];
  const int64_t d = sizes[k];
  Tails t;
  if (d >= 1 && d <= kMaxN) t = tails(0.5 * (double)d, r);
  else t.p = t.q = t.lp = t.lq = NAN;
  out[i] = t.p;
  out[m + i] = t.q;
  out[2 * m + i] = t.lp;
  out[3 * m + i] = t.lq;
}

// out [K][M]: entry m of tensor k is the r at which the tail `upper[m] ? Q : P` of a = sizes[k] / 2 equals value[m]
// (its logarithm when is_log).  A tail above 1/2 is solved on the other side, whose value 1 - v is exact for v >= 1/2.
__global__ __launch_bounds__(kThreads) void quantile_kernel(const int64_t* __restrict__ sizes, int K,
                                                            const double* __restrict__ value,
                                                            const int32_t* __restrict__ upper, int M, int is_log,
                                                            double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)K * M) return;
  const int k = (int)(i / M), m = (int)(i - (int64_t)k * M);
  const int64_t d = sizes[k];
  const double v = value[m];
  bool up = upper[m] != 0;
  double target;
  if (is_log) {
    target = v;
    if (v > num::kLogHalf && v <= 0.0) target = log(-expm1(v)), up = !up;
  } else {
    target = log(v);
    if (v > 0.5 && v <= 1.0) target = log(1.0 - v), up = !up;
  }
  if (!(target <= 0.0)) target = NAN;                       // a probability above 1
  out[i] = d >= 1 && d <= kMaxN ? tail_inverse(0.5 * (double)d, target, up) : NAN;
}

// One thread per step; workgroup b of min(tiles, kStepBlocks) takes the tiles of kThreads steps b, b + blocks, ...
// share [C][S], mean [S], se [S], totals [K][C] then the number of finite est / temperature.  The counts of a workgroup
// are kept in LDS (a wave's ballot, one LDS integer atomic per wave, tensor and level) and added to totals with one global
// integer atomic per non-zero count at its end; a table of more than kLdsCounts counts goes to totals directly.
template <typename T>
__global__ __launch_bounds__(kThreads) void steps_kernel(const T* __restrict__ est, int64_t S, int K, int64_t stride_s,
                                                         int64_t stride_k, const double* __restrict__ temperature,
                                                         int64_t temp_stride, const int64_t* __restrict__ sizes,
                                                         const double* __restrict__ bounds, int C,
                                                         double* __restrict__ share, double* __restrict__ mean,
                                                         double* __restrict__ se,
                                                         unsigned long long* __restrict__ totals, int64_t tiles) {
  __shared__ unsigned int counts[kLdsCounts];               // (a workgroup sees fewer than 2^31 (step, tensor) pairs)
  const int64_t slots = (int64_t)K * C + 1;
  const bool in_lds = C > 0 && slots <= kLdsCounts;
  if (in_lds) {
    for (int i = threadIdx.x; i < (int)slots; i += kThreads) counts[i] = 0u;
    __syncthreads();
  }
  const bool lane0 = (threadIdx.x & (warpSize - 1)) == 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
  const int64_t s = tile * kThreads + threadIdx.x;
  const bool live = s < S;
  const T* __restrict__ row = est + (live ? s : 0) * stride_s;
  if (C > 0) {                                              // (uniform: every lane of a wave walks the same k and c)
    const double temp = temperature[(live ? s : 0) * temp_stride];
    int inside[kMaxLevels];
#pragma unroll
    for (int c = 0; c < kMaxLevels; ++c) inside[c] = 0;
    for (int k = 0; k < K; ++k) {
      const double r = (double)row[k * stride_k] / temp;
      const bool fin = live && fabs(r) < INFINITY;
      const unsigned long long nf = __ballot(fin);
      if (lane0 && nf) {
        if (in_lds) atomicAdd(&counts[slots - 1], (unsigned int)__popcll(nf));
        else atomicAdd(totals + (slots - 1), (unsigned long long)__popcll(nf));
      }
#pragma unroll
      for (int c = 0; c < kMaxLevels; ++c) {
        if (c < C) {
          const double* __restrict__ b = bounds + ((int64_t)k * C + c) * 2;
          const bool in = live && b[0] <= r && r <= b[1];     // false for NaN, and for the inf of a zero temperature
          inside[c] += in ? 1 : 0;
          const unsigned long long n = __ballot(in);
          if (lane0 && n) {
            if (in_lds) atomicAdd(&counts[k * C + c], (unsigned int)__popcll(n));
            else atomicAdd(totals + ((int64_t)k * C + c), (unsigned long long)__popcll(n));
          }
        }
      }
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < kMaxLevels; ++c)
        if (c < C) share[(int64_t)c * S + s] = (double)inside[c] / (double)K;
    }
  }
  if (live && mean) {
  // Cochran (1977), plot.py's weighted_var_se:  xw = sum w x / sum w,  wb = sum w / n,
  //   se = n / ((n - 1) (sum w)^2) [sum (w x - wb xw)^2 - 2 xw sum (w x - wb xw)(w - wb) + xw^2 sum (w - wb)^2].
  // The bracket is sum ((w x - wb xw) - xw (w - wb))^2 = sum w^2 (x - xw)^2 identically, and is evaluated in that form:
  // with one tensor far larger than the others its three terms are of size (sum w x)^2 and cancel to a 1e-5th of
  // that (sizes 1 .. 36864), which costs the three-term form five or six digits in fp64.
  double sw = 0.0, cw = 0.0, sx = 0.0, cx = 0.0;
  for (int k = 0; k < K; ++k) {
    const double w = (double)sizes[k];
    num::comp_add(sw, cw, w);
    num::comp_add(sx, cx, w * (double)row[k * stride_k]);
  }
  const double n = (double)K, W = sw + cw, xw = (sx + cx) / W;
  double sa = 0.0, ca = 0.0;
  for (int k = 0; k < K; ++k) {
    const double e = (double)sizes[k] * ((double)row[k * stride_k] - xw);
    num::comp_add(sa, ca, e * e);
  }
  mean[s] = xw;
  se[s] = n / ((n - 1.0) * (W * W)) * (sa + ca);
  }
  }
  if (in_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < (int)slots; i += kThreads)
      if (counts[i]) atomicAdd(totals + i, (unsigned long long)counts[i]);
  }
}

template <typename T>
__global__ __launch_bounds__(kScan) void ewma_kernel(const T* __restrict__ x, int64_t S, int64_t stride_r,
                                                     int64_t stride_s, double alpha, double* __restrict__ y) {
  __shared__ double sA[kScan], sB[kScan];
  const int t = threadIdx.x;
  const T* __restrict__ row = x + (int64_t)blockIdx.x * stride_r;
  double* __restrict__ out = y + (int64_t)blockIdx.x * S;
  const int64_t L = (S + kScan - 1) / kScan;
  const int64_t begin = (int64_t)t * L < S ? (int64_t)t * L : S, end = begin + L < S ? begin + L : S;
  if (alpha == 0.0) {                                       // the input's bits
    for (int64_t i = begin; i < end; ++i) out[i] = (double)row[i * stride_s];
    return;
  }
  const double om = 1.0 - alpha;
  double A = 1.0, B = 0.0;                                  // the steps of this thread as one map y -> A y + B
  for (int64_t i = begin; i < end; ++i) {
    const double v = (double)row[i * stride_s];
    if (i == 0) A = 0.0, B = v;
    else B = om * v + alpha * B, A = alpha * A;
  }
  sA[t] = A;
  sB[t] = B;
  for (int off = 1; off < kScan; off <<= 1) {               // inclusive scan: thread t ends with the map of steps < end
    __syncthreads();
    double pa = 1.0, pb = 0.0;
    const bool has = t >= off;
    if (has) pa = sA[t - off], pb = sB[t - off];
    __syncthreads();
    if (has) {
      // (A = alpha^n of steps that do not contain step 0; where it has underflowed, an infinite earlier value must
      // stay infinite as it does step by step, not become 0 * inf)
      const double carried = A == 0.0 && fabs(pb) == INFINITY ? pb : A * pb;
      B = carried + B;
      A = A * pa;
      sA[t] = A;
      sB[t] = B;
    }
  }
  __syncthreads();
  double carry = t > 0 ? sB[t - 1] : 0.0;                   // (A of a prefix is 0: it contains step 0)
  for (int64_t i = begin; i < end; ++i) {
    const double v = (double)row[i * stride_s];
    carry = i == 0 ? v : om * v + alpha * carry;
    out[i] = carry;
  }
}

inline bool strided_ok(int64_t S, int K) { return S >= 1 && S <= kMaxN && K >= 1 && S * (int64_t)K <= kMaxN; }

}  // namespace temper

extern "C" int sgmcmc_temper_tails(const void* est, int is_f64, int64_t S, int K, int64_t stride_s, int64_t stride_k,
                                   const double* temperature, int64_t temp_stride, const int64_t* sizes, double* out,
                                   void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!est || !sizes || !out || !temper::strided_ok(S, K)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((S * K + temper::kThreads - 1) / temper::kThreads)), block(temper::kThreads);
  if (is_f64) SGMCMC_LAUNCH(temper::tails_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)est, S, K,
                            stride_s, stride_k, temperature, temp_stride, sizes, out);
  else SGMCMC_LAUNCH(temper::tails_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)est, S, K, stride_s,
                     stride_k, temperature, temp_stride, sizes, out);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_temper_quantile(const int64_t* sizes, int K, const double* value, const int32_t* upper, int M,
                                      int is_log, double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!sizes || !value || !upper || !out || K < 1 || M < 1 || (int64_t)K * M > temper::kMaxN)
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(((int64_t)K * M + temper::kThreads - 1) / temper::kThreads)), block(temper::kThreads);
  SGMCMC_LAUNCH(temper::quantile_kernel, grid, block, 0, (hipStream_t)stream, sizes, K, value, upper, M, is_log, out);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_temper_steps(const void* est, int is_f64, int64_t S, int K, int64_t stride_s, int64_t stride_k,
                                   const double* temperature, int64_t temp_stride, const int64_t* sizes,
                                   const double* bounds, int C, double* share, double* mean, double* se,
                                   int64_t* totals, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!est || !sizes || !temper::strided_ok(S, K) || C < 0 || C > temper::kMaxLevels || (!mean != !se) ||
      (C == 0 && !mean) || (C > 0 && (!temperature || !bounds || !share || !totals)))
    return (int)hipErrorInvalidValue;
  if (C > 0) {
    const hipError_t e = hipMemsetAsync(totals, 0, sizeof(int64_t) * ((size_t)K * C + 1), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  const int64_t tiles = (S + temper::kThreads - 1) / temper::kThreads;
  const dim3 grid((unsigned)(tiles < temper::kStepBlocks ? tiles : temper::kStepBlocks)), block(temper::kThreads);
  if (is_f64) SGMCMC_LAUNCH(temper::steps_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)est, S, K,
                            stride_s, stride_k, temperature, temp_stride, sizes, bounds, C, share, mean, se,
                            (unsigned long long*)totals, tiles);
  else SGMCMC_LAUNCH(temper::steps_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)est, S, K, stride_s,
                     stride_k, temperature, temp_stride, sizes, bounds, C, share, mean, se,
                     (unsigned long long*)totals, tiles);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_temper_ewma(const void* x, int is_f64, int R, int64_t S, int64_t stride_r, int64_t stride_s,
                                  double alpha, double* y, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !y || R < 1 || !temper::strided_ok(S, R) || !(alpha >= 0.0 && alpha < 1.0)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)R), block(temper::kScan);
  if (is_f64) SGMCMC_LAUNCH(temper::ewma_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x, S,
                            stride_r, stride_s, alpha, y);
  else SGMCMC_LAUNCH(temper::ewma_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, S, stride_r,
                     stride_s, alpha, y);
  return (int)hipGetLastError();
}
