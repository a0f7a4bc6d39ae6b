// Uncertainty decomposition of a posterior ensemble and risk-coverage curves (evaluation side, fp64, deterministic; the
// reference has neither).  Two kernels:
//
//   rows_kernel  one pass over acc [E][N][C]: calib::ensemble_kernel's (row, class) layout and its very log-sum-exp and
//                softmax (num::lse_add4 / lse_add1 / lse_log_mean / row_softmax), so probs / max_prob / pred / hit are
//                its bits.  Beside the running log-sum-exp a thread keeps sum_e p log p of its class, on the same running
//                maximum and from the same exponentials (one exp per entry, as in ensemble_kernel); the four samples
//                of a step are also handed over through LDS so that thread (row, j) finds the first argmax of sample j
//                of that row and counts it in an integer vote table (one writer per entry: no atomics).  The row's
//                thread then finishes margin, entropy, expected entropy, mutual information, disagreement, nll, brier.
//   risk_kernel  one workgroup over the rows ranked from the most confident down: tie groups by block scans (as
//                calib::rank_kernel), prefix sums of the losses, the tie-averaged risk at every coverage and its mean.
//
// Every sum runs in an order fixed by the sizes alone; counts are integers.  No atomics, no host round trip.

namespace uncert {

constexpr int kPlane = 258;        // doubles between the four samples' planes of a hand-over buffer: 2 past 256, so
                                   // that the four readers of a row sit on different LDS banks

// x exp(x - m) for the term t = exp(x - m) the log-sum-exp has just formed (0 where x = -inf; a NaN stays a NaN)
__device__ __forceinline__ double x_times(double x, double t) { return x == -INFINITY ? 0.0 : t * x; }

__global__ __launch_bounds__(256) void rows_kernel(const double* __restrict__ acc, const int64_t* __restrict__ labels,
                                                   int E, int N, int C, double* __restrict__ probs,
                                                   double* __restrict__ conf, int64_t* __restrict__ pred,
                                                   int64_t* __restrict__ hit, double* __restrict__ margin,
                                                   double* __restrict__ entropy, double* __restrict__ expected,
                                                   double* __restrict__ mutual, double* __restrict__ disagree,
                                                   double* __restrict__ nll, double* __restrict__ brier) {
  __shared__ double row[256], hsum[256];
  __shared__ double xs[2][4 * kPlane];           // two hand-over buffers: one barrier per step
  __shared__ int votes[4][256];                  // votes[j][r * C + c]: samples e = j (mod 4) of row r with argmax c
  const int rows = 256 / C;
  const int t = threadIdx.x, r = t / C, c = t - r * C;
  const int64_t n0 = (int64_t)blockIdx.x * rows;
  const bool live = r < rows && n0 + r < N;
  const size_t plane = (size_t)N * C;
  const double* __restrict__ a = acc + (live ? (size_t)(n0 + r) * C + c : 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) votes[j][t] = 0;
  // (m, s): the running log-sum-exp; g = sum_e x_e exp(x_e - m) rides on the same maximum and takes the same factor
  // when it moves, so that sum_e p log p = exp(m) g costs no second exp per entry
  double m = -INFINITY, s = 0.0, g = 0.0;
  double x[4] = {0.0, 0.0, 0.0, 0.0}, nx[4] = {0.0, 0.0, 0.0, 0.0};
  if (live && E >= 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = a[(size_t)j * plane];
  }
  int buf = 0;
  for (int e = 0; e < E; e += 4, buf ^= 1) {
    const int cnt = min(4, E - e);                // 4, or the 1 .. 3 samples of the tail
    double* xb = xs[buf];
    if (cnt == 4) {
      if (live && e + 8 <= E) {                   // the next step's loads fly across this step's barrier
#pragma unroll
        for (int j = 0; j < 4; ++j) nx[j] = a[(size_t)(e + 4 + j) * plane];
      }
      if (live) {
        double f, tm[4];
        num::lse_add4(m, s, x[0], x[1], x[2], x[3], f, tm);
        g = g * f;
        g = (((g + x_times(x[0], tm[0])) + x_times(x[1], tm[1])) + x_times(x[2], tm[2])) + x_times(x[3], tm[3]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { xb[j * kPlane + t] = x[j]; x[j] = nx[j]; }
    } else {
      for (int j = 0; j < cnt; ++j) {
        double v = 0.0;
        if (live) {
          double f, tm;
          v = a[(size_t)(e + j) * plane];
          num::lse_add1(m, s, v, f, tm);
          g = g * f + x_times(v, tm);
        }
        xb[j * kPlane + t] = v;
      }
    }
    __syncthreads();
    for (int task = t; task < 4 * rows; task += 256) {      // task = (row vr, sample vj): one pass for C >= 4
      const int vr = task >> 2, vj = task & 3;
      if (n0 + vr >= N || vj >= cnt) continue;
      const double* v = xb + vj * kPlane + vr * C;
      double best = v[0];
      int arg = 0;
      for (int k = 1; k < C; ++k) {
        const double w = v[k];
        if (w > best) { best = w; arg = k; }
      }
      votes[vj][vr * C + arg] += 1;
    }
  }
  if (live) {
    row[t] = num::lse_log_mean(m, s, E);
    hsum[t] = m == -INFINITY ? g : exp(m) * g;    // sum_e p log p of this class (g = 0 where every sample has p = 0)
  }
  __syncthreads();
  const int64_t n = n0 + t;
  if (t < rows && n < N) {
    double* l = row + t * C;
    num::row_softmax(l, C, probs + n * C);
    num::row_max(l, C, n, labels, conf, pred, hit);
    const double top = conf[n];
    const int arg = (int)pred[n];
    double second = C == 1 ? 0.0 : -INFINITY, ent = 0.0, ent_c = 0.0, exp_ent = 0.0, exp_c = 0.0;
    for (int k = 0; k < C; ++k) {
      const double p = l[k];
      if (k != arg && p > second) second = p;     // the largest of the others: duplicates of the maximum count
      num::comp_add(ent, ent_c, p == 0.0 ? 0.0 : p * log(p));
      num::comp_add(exp_ent, exp_c, hsum[t * C + k]);
    }
    ent = -(ent + ent_c);
    exp_ent = -(exp_ent + exp_c) / (double)E;
    const double gap = ent - exp_ent;
    const int same = ((votes[0][t * C + arg] + votes[1][t * C + arg]) + votes[2][t * C + arg]) + votes[3][t * C + arg];
    margin[n] = top - second;                     // NaN row: every probability is NaN, so is this
    entropy[n] = ent;
    expected[n] = exp_ent;
    mutual[n] = gap < 0.0 ? 0.0 : gap;            // (a NaN is not < 0 and stays)
    disagree[n] = top != top ? top : (double)(E - same) / (double)E;
    if (labels) {
      const int64_t y = labels[n];
      const double py = y >= 0 && y < C ? l[y] : 0.0;      // a label outside 0 .. C-1 names a class of probability 0
      double b = 0.0;
      for (int k = 0; k < C; ++k) {
        const double d = l[k] - (k == y ? 1.0 : 0.0);
        b += d * d;
      }
      nll[n] = -log(py);
      brier[n] = b;
    }
  }
}

constexpr int kRiskThreads = 1024;
constexpr int kNone = 0x7fffffff;

// scores [n] (higher = more confident), losses [n], perm = sgmcmc_stable_order of scores.  Rank i = 0 .. n-1 counts from
// the most confident row down: row perm[n - 1 - i].  risk [n] and out[3] = {aurc, mean loss, has_nan} as the header
// defines them.  P(i) = the sum of the losses of ranks < i = (the scanned totals of the chunks before i's) + (the partial
// sum of i's chunk, from its first rank), formed by that one expression wherever it is needed.
__global__ __launch_bounds__(kRiskThreads) void risk_kernel(const double* __restrict__ scores,
                                                            const double* __restrict__ losses,
                                                            const int32_t* __restrict__ perm, int n,
                                                            double* __restrict__ risk, double* __restrict__ out) {
  __shared__ int first_s[kRiskThreads], last_s[kRiskThreads];
  __shared__ double incl[kRiskThreads], before_first[kRiskThreads], before_last[kRiskThreads], part[kRiskThreads];
  const int t = threadIdx.x;
  auto row_at = [&](int i) { return min(max(perm[n - 1 - i], 0), n - 1); };
  auto score_at = [&](int i) { return scores[row_at(i)]; };
  auto starts = [&](int i) { return i == 0 || score_at(i) != score_at(i - 1); };   // a tie group begins at rank i
  // thread t owns the ranks [k0, k1)
  const int L = (n + kRiskThreads - 1) / kRiskThreads;
  const int k0 = min(t * L, n), k1 = min(k0 + L, n);
  int fs = kNone, ls = -1, bad = 0;
  double run = 0.0, bf = 0.0, bl = 0.0;
  for (int i = k0; i < k1; ++i) {
    if (starts(i)) {
      if (fs == kNone) { fs = i; bf = run; }
      ls = i;
      bl = run;
    }
    const double v = losses[row_at(i)];
    bad |= v != v;
    run += v;
  }
  const double top = scores[min(max(perm[n - 1], 0), n - 1)];     // NaN sorts last in the ascending order
  bad |= top != top;
  if (__syncthreads_or(bad)) {
    const double q = num::qnan();
    for (int i = k0; i < k1; ++i) risk[i] = q;
    if (t == 0) { out[0] = q; out[1] = q; out[2] = 1.0; }
    return;
  }
  first_s[t] = fs;
  last_s[t] = ls;
  incl[t] = run;
  before_first[t] = bf;
  before_last[t] = bl;
  __syncthreads();
  num::block_scan<int, num::Min, true, kRiskThreads>(first_s, num::Min());       // the first group start in chunks >= t
  num::block_scan<int, num::Max, false, kRiskThreads>(last_s, num::Max());       // the last group start in chunks <= t
  num::block_scan<double, num::Add, false, kRiskThreads>(incl, num::Add());      // the losses of chunks <= t
  auto excl = [&](int chunk) { return chunk ? incl[chunk - 1] : 0.0; };
  const double total = incl[kRiskThreads - 1];    // P(n)
  const int nxt = t + 1 < kRiskThreads ? first_s[t + 1] : kNone;
  const double base = excl(t);
  int a = 0, b = 0;                               // the current group's ranks [a, b) and P(a), P(b)
  double Pa = 0.0, Pb = 0.0, sum = 0.0;
  run = 0.0;
  for (int i = k0; i < k1; ++i) {
    const bool st = starts(i);
    if (st || i == k0) {
      if (st) {
        a = i;
        Pa = base + run;
      } else {                                    // the group began in an earlier chunk, at that chunk's last start
        a = last_s[t - 1];
        const int owner = a / L;
        Pa = excl(owner) + before_last[owner];
      }
      double ahead = run;
      int j = i;
      do { ahead += losses[row_at(j)]; ++j; } while (j < k1 && !starts(j));
      if (j < k1) {
        b = j;
        Pb = base + ahead;
      } else if (nxt != kNone) {                  // ... and ends at a later chunk's first start
        b = nxt;
        const int owner = b / L;
        Pb = excl(owner) + before_first[owner];
      } else {
        b = n;
        Pb = total;
      }
    }
    // cum(k) = P(a) + (k - a) (P(b) - P(a)) / (b - a) at k = i + 1, over k: one division, of
    // (b - a) P(a) + (k - a) (P(b) - P(a)) by (b - a) k.  Integer-valued losses make the numerator and the denominator
    // exact, and the quotient the correctly rounded risk.  (Equal ends add nothing: also where both are +inf.)
    const double g = (double)(b - a), k = (double)(i + 1), grp = Pb == Pa ? 0.0 : Pb - Pa;
    const double rk = (g * Pa + (k - (double)a) * grp) / (g * k);
    risk[i] = rk;
    sum += rk;
    run += losses[row_at(i)];
  }
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int q = 0; q < kRiskThreads; ++q) s += part[q];
    out[0] = s / (double)n;
    out[1] = total / (double)n;
    out[2] = 0.0;
  }
}

}  // namespace uncert

extern "C" int sgmcmc_uncertainty_rows(const double* acc, const int64_t* labels, int samples, int rows, int classes,
                                       double* probs, double* max_prob, int64_t* pred, int64_t* hit, double* margin,
                                       double* entropy, double* expected_entropy, double* mutual_info,
                                       double* disagreement, double* nll, double* brier, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const bool with = labels != nullptr;
  if (!acc || !probs || !max_prob || !pred || !margin || !entropy || !expected_entropy || !mutual_info ||
      !disagreement || with != (hit != nullptr) || with != (nll != nullptr) || with != (brier != nullptr) ||
      samples <= 0 || rows <= 0 || classes <= 0 || classes > calib::kMaxClasses)
    return (int)hipErrorInvalidValue;
  const int per = 256 / classes;
  SGMCMC_LAUNCH(uncert::rows_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(256), 0, (hipStream_t)stream, acc,
                labels, samples, rows, classes, probs, max_prob, pred, hit, margin, entropy, expected_entropy, mutual_info,
                disagreement, nll, brier);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_risk_coverage(const double* scores, const double* losses, const int32_t* perm, int n, double* risk,
                                    double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!scores || !losses || !perm || !risk || !out || n <= 0 || n > calib::kMaxRows) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(uncert::risk_kernel, dim3(1), dim3(uncert::kRiskThreads), 0, (hipStream_t)stream, scores, losses, perm,
                n, risk, out);
  return (int)hipGetLastError();
}
