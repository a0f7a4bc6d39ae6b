// The fp64 numerics that the statistics kernels (calib_hip.inc .. raob_hip.inc) share, included once from sgmcmc_hip.hip
// before the first of them: a feature file depends on this file and on data-layout types, never on another feature
// file's arithmetic.  Built with -ffp-contract=off and without fast-math, a function's result is fixed by the order of
// its operations and its literals; the callers are held to fp64 references within a few eps, so a changed operation
// here changes every caller's bits at once.
#pragma once

namespace num {

// ---- constants ----------------------------------------------------------------------------------------------------------
constexpr double kHalfLog2Pi = 0.91893853320467274178;      // log(2 pi) / 2
constexpr double kTwoPi = 6.283185307179586477;
constexpr double kInvSqrt2 = 0.70710678118654752440;
constexpr double kLogHalf = -0.69314718055994530942;
constexpr double kInvSqrtPi = 0.56418958354775628695;
constexpr double kInvSqrt2Pi = 0.39894228040143267794;

// ---- small helpers ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ bool is_finite(double v) { return fabs(v) < INFINITY; }         // false for NaN as well

// s + c += v, c collecting what each addition rounds away (Neumaier): a long sum stays within an ulp or two of its exact
// value, in a fixed order
__device__ __forceinline__ void comp_add(double& s, double& c, double v) {
  const double t = s + v;
  c += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
  s = t;
}

// a + b exactly: the rounded sum, and what the rounding lost (Knuth)
__device__ __forceinline__ double two_sum(double a, double b, double& err) {
  const double s = a + b, bb = s - a;
  err = (a - (s - bb)) + (b - bb);
  return s;
}

// ---- log-sum-exp accumulators -------------------------------------------------------------------------------------------
// one term of a running sum_e exp(x_e - m): a NaN survives an all -inf column
__device__ __forceinline__ double lse_term(double x, double m) {
  return m == -INFINITY ? (x != x ? x : 0.0) : exp(x - m);
}

// The running log-sum-exp over the samples of one (row, class) entry, (m, s) with sum_e exp(x_e) = s exp(m): four
// samples at a time, then one at a time, then the log-mean.  calib::ensemble_kernel and uncert::rows_kernel both run
// exactly this sequence, which is what makes their probabilities the same bits.
// (f: the factor s took when the maximum moved, 1 otherwise; t[i]: the term exp(x_i - m) that was added -- for a caller
// that carries a second sum on the same maximum)
__device__ __forceinline__ void lse_add4(double& m, double& s, double x0, double x1, double x2, double x3, double& f,
                                         double* t) {
  const double mx = fmax(fmax(m, fmax(x0, x1)), fmax(x2, x3));
  f = 1.0;
  if (mx > m) {
    if (m != -INFINITY) { f = exp(m - mx); s = s * f; }
    m = mx;
  }
  t[0] = lse_term(x0, m); t[1] = lse_term(x1, m); t[2] = lse_term(x2, m); t[3] = lse_term(x3, m);
  s = (((s + t[0]) + t[1]) + t[2]) + t[3];
}

__device__ __forceinline__ void lse_add1(double& m, double& s, double x, double& f, double& t) {
  f = 1.0;
  if (x > m) {
    if (m != -INFINITY) { f = exp(m - x); s = s * f; }
    m = x;
  }
  t = lse_term(x, m);
  s += t;
}

__device__ __forceinline__ void lse_add4(double& m, double& s, double x0, double x1, double x2, double x3) {
  double f, t[4];
  lse_add4(m, s, x0, x1, x2, x3, f, t);
}
__device__ __forceinline__ void lse_add1(double& m, double& s, double x) {
  double f, t;
  lse_add1(m, s, x, f, t);
}
__device__ __forceinline__ double lse_log_mean(double m, double s, int E) { return (m + log(s)) - log((double)E); }

// softmax of the C log-means in l (LDS), in place and to p (global): the ensemble's probabilities of one row
__device__ __forceinline__ void row_softmax(double* l, int C, double* __restrict__ p) {
  double mx = l[0];
  for (int k = 1; k < C; ++k) mx = fmax(mx, l[k]);
  double s = 0.0;
  for (int k = 0; k < C; ++k) { l[k] = exp(l[k] - mx); s += l[k]; }
  for (int k = 0; k < C; ++k) { l[k] = l[k] / s; p[k] = l[k]; }
}

// max-prob, first index of the maximum (np.argmax: a NaN wins and the first NaN is kept) and hit of one row
__device__ __forceinline__ void row_max(const double* p, int C, int64_t n, const int64_t* __restrict__ labels,
                                        double* __restrict__ conf, int64_t* __restrict__ pred,
                                        int64_t* __restrict__ hit) {
  double best = p[0];
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const double v = p[c];
    if (v > best || (v != v && best == best)) { best = v; arg = c; }
  }
  conf[n] = best;
  pred[n] = arg;
  if (hit) hit[n] = (labels[n] == (int64_t)arg) ? 1 : 0;
}

// ---- logarithm and gamma helpers ----------------------------------------------------------------------------------------
// log1p(u) - u, u > -1: for |u| <= 0.5 as -r u + 2 r^3 (1/3 + r^2/5 + r^4/7 + ...), r = u / (2 + u), which has no
// cancellation (-r u is the whole second-order term)
__device__ __forceinline__ double log1p_minus(double u) {
  if (fabs(u) > 0.5) return log1p(u) - u;
  const double r = u / (2.0 + u), r2 = r * r;
  double power = 1.0, series = 1.0 / 3.0;
  for (int k = 5; k < 80; k += 2) {
    power *= r2;
    const double term = power / (double)k;
    series += term;
    if (term < 1e-18 * series) break;
  }
  return 2.0 * r * r2 * series - r * u;
}

// digamma and trigamma for x > 0: the recurrence up to x >= 10, then the asymptotic series through B_14 (the first
// term left out is below 5e-17 there)
__device__ __forceinline__ double digamma(double x) {
  double r = 0.0;
  while (x < 10.0) { r -= 1.0 / x; x += 1.0; }
  const double f = 1.0 / (x * x);
  const double t = f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132
                   - f * (691.0 / 32760 - f * (1.0 / 12)))))));
  return r + (log(x) - 0.5 / x - t);
}
__device__ __forceinline__ double trigamma(double x) {
  double r = 0.0;
  while (x < 10.0) { r += 1.0 / (x * x); x += 1.0; }
  const double f = 1.0 / (x * x);
  const double t = (f / x) * (1.0 / 6 - f * (1.0 / 30 - f * (1.0 / 42 - f * (1.0 / 30 - f * (5.0 / 66
                   - f * (691.0 / 2730 - f * (7.0 / 6)))))));
  return r + (1.0 / x + 0.5 * f + t);
}

// log Gamma(x) for x > 0: lgamma(x) = lgamma(x + k) - log(x (x + 1) .. (x + k - 1)) up to x + k >= 10, then Stirling's
// series through B_14
__device__ __forceinline__ double log_gamma(double x) {
  double prod = 1.0;
  while (x < 10.0) { prod *= x; x += 1.0; }
  const double f = 1.0 / (x * x);
  const double t = (1.0 / x) * (1.0 / 12 - f * (1.0 / 360 - f * (1.0 / 1260 - f * (1.0 / 1680 - f * (1.0 / 1188
                   - f * (691.0 / 360360 - f * (1.0 / 156)))))));
  return (((x - 0.5) * log(x) - x) + kHalfLog2Pi + t) - log(prod);
}

// Stirling's remainder D(z) = lgamma(z) - ((z - 1/2) log z - z + log(2 pi) / 2) = 1/(12 z) - 1/(360 z^3) + ..., z > 0,
// in the two forms the callers were measured with:
//   stirling_rest_lgamma  the series from z = kStirling = 20 on and the difference itself below (where lgamma is small
//                         and the difference costs nothing).  Callers: make_beta, i.e. the incomplete beta function of
//                         summary::mcse_quantile_kernel.
//   stirling_rest         log_gamma's series from z >= 10 on, the recurrence D(z) = D(z + 1) + (z + 1/2) log1p(1 / z) - 1
//                         below.  Callers: gof::prepare (the t, gennorm and dgamma families) and temper::tails.
// They agree to rounding, not to the bit: merging them changes results and is not part of what moved them here.
constexpr double kStirling = 20.0;

__device__ __forceinline__ double stirling_rest_lgamma(double z) {
  if (z < kStirling) return lgamma(z) - ((z - 0.5) * log(z) - z + kHalfLog2Pi);
  const double r = 1.0 / z, r2 = r * r;
  return r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0 - r2 * (1.0 / 1188.0 - r2 * (691.0 / 360360.0))))));
}

__device__ double stirling_rest(double a) {
  double d = 0.0;
  while (a < 10.0) {                                  // D(a) - D(a + 1) = (a + 1/2) log1p(1 / a) - 1
    const double v = 1.0 / a;
    d += v <= 0.5 ? (a + 0.5) * log1p_minus(v) + 0.5 * v : (a + 0.5) * log1p(v) - 1.0;
    a += 1.0;
  }
  const double f = 1.0 / (a * a);                     // log_gamma's series
  return d + (1.0 / a) * (1.0 / 12 - f * (1.0 / 360 - f * (1.0 / 1260 - f * (1.0 / 1680 - f * (1.0 / 1188
             - f * (691.0 / 360360 - f * (1.0 / 156)))))));
}

// ---- the regularised incomplete gamma function --------------------------------------------------------------------------
// P(a, x) = prefactor * gamma_series (meant for x < a + 1) and Q(a, x) = prefactor * gamma_fraction (for x >= a + 1),
// prefactor = x^a e^-x / Gamma(a): the caller forms it, as a logarithm, and chooses the region.  Both need O(sqrt a)
// terms near x = a; max_terms caps a loop that has ended long before.  The series is sum_k x^k / (a (a + 1) .. (a + k)),
// the fraction the continued fraction of Q by the modified Lentz recurrence.
__device__ __forceinline__ double gamma_series(double a, double x, int max_terms) {
  double ap = a, term = 1.0 / a, sum = term;
  for (int k = 0; k < max_terms; ++k) {
    ap += 1.0;
    term *= x / ap;
    sum += term;
    if (term <= 1.1e-16 * sum) break;
  }
  return sum;
}
__device__ __forceinline__ double gamma_fraction(double a, double x, int max_terms) {
  constexpr double tiny = 1e-300;
  double b = x + 1.0 - a, cc = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int i = 1; i <= max_terms; ++i) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < tiny) d = tiny;
    cc = b + an / cc;
    if (fabs(cc) < tiny) cc = tiny;
    d = 1.0 / d;
    const double del = d * cc;
    h *= del;
    if (fabs(del - 1.0) <= 2.3e-16) break;
  }
  return h;
}

// ---- the bracketed Newton step ------------------------------------------------------------------------------------------
// A root search on a monotone function: the caller moves lo or hi to the iterate x by the sign it found there (every
// evaluation narrows the bracket) and forms its own Newton step; advance() keeps that step inside the bracket and
// returns false when the search is over.  While hi is infinite a step grows x eightfold at most (a flat function sends
// it anywhere).  The first Newton step below 1e-10 x is the last: its successor would be about 1e-20 x |f''| x / (2 f').
struct Bracket {
  double lo, hi;
  __device__ __forceinline__ bool advance(double& x, double next) {
    if (next == x) return false;                                       // a Newton step below half an ulp
    if (!(hi < INFINITY) && next > 8.0 * x) next = 8.0 * x;
    const bool newton = next > lo && next < hi;
    if (!newton) next = hi < INFINITY ? 0.5 * (lo + hi) : 2.0 * x;
    if (next == lo || next == hi) return false;                        // the bracket has no interior left
    const bool last = newton && fabs(next - x) <= 1e-10 * x;
    x = next;
    return !last;
  }
};

// ---- the regularised incomplete beta function I_x(a, b) and its inverse -------------------------------------------------
// I_x(a, b) = front(x) cf(x; a, b) / a for x < (a + 1) / (a + b + 2), else 1 - front(x) cf(1 - x; b, a) / b, with
// front(x) = x^a (1 - x)^b / B(a, b) and cf the continued fraction 26.5.8 of Abramowitz and Stegun by the modified Lentz
// recurrence.  The accuracy of I at a, b of 10^4 is that of log front: lgamma(a + b) - lgamma(a) - lgamma(b) loses
// log10(a log a) digits, so Stirling's formula is applied to the three of them on paper and only its remainders D are
// evaluated (TOMS 708's brcomp),
//   log front = a l(u) + b l(w) + log(a b / (2 pi T)) / 2 + D(T) - D(a) - D(b),   l(u) = log1p(u) - u,
//   T = a + b,  u = (x T - a) / a,  w = -(x T - a) / b   (a u + b w = 0 exactly: the first-order terms cancel on paper),
//   D = stirling_rest_lgamma,
// and T carried as the rounded sum and its rounding error so that x T - a is formed with one rounding.
constexpr int kBetaFractionTerms = 4000, kBetaEvenTerms = 20000, kBetaRootSteps = 200;      // at most

struct Beta {               // a, b and what does not depend on x
  double a, b, total, total_err, log_const;
};

__device__ __forceinline__ Beta make_beta(double a, double b) {
  Beta B;
  B.a = a;
  B.b = b;
  B.total = two_sum(a, b, B.total_err);                           // total + total_err = a + b exactly
  B.log_const = 0.5 * log(a * b / (kTwoPi * B.total)) + stirling_rest_lgamma(B.total) - stirling_rest_lgamma(a) -
                stirling_rest_lgamma(b);
  return B;
}

// x^a (1 - x)^b / B(a, b), 0 < x < 1
__device__ __forceinline__ double beta_front(const Beta& B, double x) {
  const double excess = fma(x, B.total, -B.a) + x * B.total_err;      // x T - a
  const double u = excess / B.a, w = -excess / B.b;
  if (!(u > -1.0 && w > -1.0)) return 0.0;
  return exp(B.a * log1p_minus(u) + B.b * log1p_minus(w) + B.log_const);
}

__device__ double beta_fraction(double a, double b, double x) {
  constexpr double tiny = 1e-300;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= kBetaFractionTerms; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= 2.3e-16) break;
  }
  return h;
}

// I_x(a, b) / (x^a y^b / B(a, b)), y = 1 - x, for x below the mean: the EVEN PART of the continued fraction that
// beta_fraction evaluates (DiDonato & Morris 1992, TOMS 708, BFRAC), in x, y and lambda = (a + b) y - b, each given with
// one rounding.  The plain fraction forms 1 - (a + b) x / (a + 1) and its likes from x alone: where y is small (the t
// family of gof at df large: y = 5e-4 at df = 1e4, z = 2) they cancel and cost 1 / y roundings, measured 313 eps at
// df = 1e4; the contraction carries that difference as lambda and loses nothing (measured below 6 eps for df = 0.1 .. 1e4).
__device__ double beta_fraction_even(double a, double b, double x, double y, double lambda) {
  const double c = lambda + 1.0, c0 = b / a, c1 = 1.0 / a + 1.0, yp1 = y + 1.0;
  double n = 0.0, p = 1.0, s = a + 1.0, an = 0.0, bn = 1.0, anp1 = 1.0, bnp1 = c / c1, r = c1 / c;
  for (int it = 0; it < kBetaEvenTerms; ++it) {
    n += 1.0;
    double t = n / a;
    const double w = n * (b - n) * x;
    double e = a / s;
    const double alpha = p * (p + c0) * e * e * (w * x);
    e = (t + 1.0) / (c1 + t + t);
    const double beta = n + w / s + e * (c + n * yp1);
    p = t + 1.0;
    s += 2.0;
    t = alpha * an + beta * anp1;
    an = anp1;
    anp1 = t;
    t = alpha * bn + beta * bnp1;
    bn = bnp1;
    bnp1 = t;
    const double r0 = r;
    r = anp1 / bnp1;
    if (fabs(r - r0) <= 1e-16 * r) break;
    an /= bnp1;                                             // rescaled: b_(n + 1) = 1
    bn /= bnp1;
    anp1 = r;
    bnp1 = 1.0;
  }
  return r;
}

// I_x(a, b) and the density x^(a-1) (1 - x)^(b-1) / B(a, b), 0 < x < 1
__device__ double beta_cdf(const Beta& B, double x, double* density) {
  const double front = beta_front(B, x);
  *density = front / (x * (1.0 - x));
  if (x < (B.a + 1.0) / (B.total + 2.0)) return front * beta_fraction(B.a, B.b, x) / B.a;
  return 1.0 - front * beta_fraction(B.b, B.a, 1.0 - x) / B.b;
}

// the x in (0, 1) with I_x(a, b) = P, 0 < P < 1, a, b > 0, by Bracket (hi = 1: a bisection step whenever Newton leaves
// the bracket or the density vanishes), from `sds` standard deviations of the beta distribution off its mean (P =
// Phi(sds)); at the last step |f''| x / (2 f') is x / sd <= sqrt(a + b) that close to the mean.
__device__ double beta_inverse(const Beta& B, double P, double sds) {
  const double mean = B.a / B.total;
  Bracket br = {0.0, 1.0};
  double x = mean + sds * sqrt(mean * (B.b / B.total) / (B.total + 1.0));
  if (!(x > br.lo && x < br.hi)) x = mean;
  for (int it = 0; it < kBetaRootSteps; ++it) {
    double density;
    const double f = beta_cdf(B, x, &density) - P;
    if (f == 0.0) return x;
    if (f < 0.0) br.lo = x;
    else br.hi = x;
    if (!br.advance(x, x - f / density)) break;
  }
  return x;
}

// ---- the normal quantile ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double polevl(double x, const double* c, int n) {
  double a = c[0];
  for (int i = 1; i <= n; ++i) a = a * x + c[i];
  return a;
}

// the inverse of the standard normal distribution function, 0 < y0 < 1: Cephes' ndtri (three rational approximations)
__device__ double ndtri(double y0) {
  constexpr double s2pi = 2.50662827463100050242E0, expm2 = 0.13533528323661269189;
  const double P0[5] = {-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1,
                        1.39312609387279679503E1, -1.23916583867381258016E0};
  const double Q0[9] = {1.00000000000000000000E0, 1.95448858338141759834E0, 4.67627912898881538453E0,
                        8.63602421390890590575E1, -2.25462687854119370527E2, 2.00260212380060660359E2,
                        -8.20372256168333339912E1, 1.59056225126211695515E1, -1.18331621121330003142E0};
  const double P1[9] = {4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1,
                        4.40805073893200834700E1, 1.46849561928858024014E1, 2.18663306850790267539E0,
                        -1.40256079171354495875E-1, -3.50424626827848203418E-2, -8.57456785154685413611E-4};
  const double Q1[9] = {1.00000000000000000000E0, 1.57799883256466749731E1, 4.53907635128879210584E1,
                        4.13172038254672030440E1, 1.50425385692907503408E1, 2.50464946208309415979E0,
                        -1.42182922854787788574E-1, -3.80806407691578277194E-2, -9.33259480895457427372E-4};
  const double P2[9] = {3.23774891776946035970E0, 6.91522889068984211695E0, 3.93881025292474443415E0,
                        1.33303460815807542389E0, 2.01485389549179081538E-1, 1.23716634817820021358E-2,
                        3.01581553508235416007E-4, 2.65806974686737550832E-6, 6.23974539184983293730E-9};
  const double Q2[9] = {1.00000000000000000000E0, 6.02427039364742014255E0, 3.67983563856160859403E0,
                        1.37702099489081330271E0, 2.16236993594496635890E-1, 1.34204006088543189037E-2,
                        3.28014464682127739104E-4, 2.89247864745380683936E-6, 6.79019408009981274425E-9};
  bool negate = true;
  double y = y0;
  if (y > 1.0 - expm2) {
    y = 1.0 - y;
    negate = false;
  }
  if (y > expm2) {
    y = y - 0.5;
    const double y2 = y * y;
    const double x = y + y * (y2 * polevl(y2, P0, 4) / polevl(y2, Q0, 8));
    return x * s2pi;
  }
  double x = sqrt(-2.0 * log(y));
  const double x0 = x - log(x) / x;
  const double z = 1.0 / x;
  const double x1 = x < 8.0 ? z * polevl(z, P1, 8) / polevl(z, Q1, 8) : z * polevl(z, P2, 8) / polevl(z, Q2, 8);
  x = x0 - x1;
  return negate ? -x : x;
}

// ---- block primitives ---------------------------------------------------------------------------------------------------
struct Add { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Min { __device__ int operator()(int a, int b) const { return min(a, b); } };
struct Max { __device__ int operator()(int a, int b) const { return max(a, b); } };

// Hillis-Steele scan over one value per thread of a workgroup of kThreads, in place: inclusive from the front, or (kBack)
// from the back.  A thread without a neighbour at the distance keeps its value.  Called by the whole workgroup.
template <typename T, typename Op, bool kBack, int kThreads>
__device__ __forceinline__ void block_scan(T* buf, Op op) {
  const int t = threadIdx.x;
  for (int off = 1; off < kThreads; off <<= 1) {
    const int o = kBack ? t + off : t - off;
    const bool has = o >= 0 && o < kThreads;
    const T v = has ? buf[o] : buf[t];
    __syncthreads();
    if (has) buf[t] = kBack ? op(buf[t], v) : op(v, buf[t]);
    __syncthreads();
  }
}

// the sum of f(i), i < N, in an order fixed by N: thread t of kThreads adds i = t, t + kThreads, ... ascending, then a
// tree over threads.  sh: kThreads doubles of LDS.  Called by the whole workgroup.
template <int kThreads, typename F>
__device__ double block_sum(int64_t N, double* sh, F f) {
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += kThreads) a = __dadd_rn(a, f(i));
  __syncthreads();
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w /= 2) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = __dadd_rn(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  return sh[0];
}

// The compare-exchange walk of the column sorts (summary::sort_kernel, powerscale::sort_kernel): a bitonic network along
// the rows of an LDS tile [n_pad][1 << log_tq] (n_pad a power of two), every column ascending.  q is the fastest index of
// the tile AND of the thread numbering: a step with distance j pairs row i (bit j clear) with row i + j, thread p takes
// column p % TQ of pair p / TQ, so no lane group strides along the rows (summary_hip.inc has the bank argument).
// kKeyed: key [n_pad][TQ] travels with its value and breaks ties, the smaller key first -- with distinct keys a total
// order, so the result does not depend on the network.  Without keys equal values are interchangeable.  Called by the
// whole workgroup after the tile is written (the walk begins with a barrier); the caller synchronises before reading.
template <bool kKeyed, int kThreads>
__device__ __forceinline__ void bitonic_walk(double* __restrict__ tile, uint16_t* __restrict__ key, int n_pad,
                                             int log_tq) {
  const int t = threadIdx.x, tq = 1 << log_tq;
  const int pairs = (n_pad << log_tq) >> 1;
  for (int k = 2; k <= n_pad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int p = t; p < pairs; p += kThreads) {
        const int c = p & (tq - 1), pr = p >> log_tq;
        const int i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1));        // bit j clear; the partner is i + j
        const int lo = (i << log_tq) | c, hi = ((i | j) << log_tq) | c;
        const double a = tile[lo], b = tile[hi];
        const bool ascending = (i & k) == 0;                           // always in the last merge, k = n_pad
        if constexpr (kKeyed) {
          const uint16_t ka = key[lo], kb = key[hi];
          const bool above = a > b || (a == b && ka > kb), below = a < b || (a == b && ka < kb);
          if (ascending ? above : below) {
            tile[lo] = b;
            tile[hi] = a;
            key[lo] = kb;
            key[hi] = ka;
          }
        } else {
          if (ascending ? a > b : a < b) {
            tile[lo] = b;
            tile[hi] = a;
          }
        }
      }
    }
  }
}

}  // namespace num
