// Posterior summaries of stored draws with their Monte Carlo standard errors: mean, sd, quantiles, the highest-density
// interval, and the MCSE of the mean, the sd and every quantile (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; the R
// package posterior; ArviZ's unimodal HDI).  include/sgmcmc_hip.h states the definition.  The effective sample sizes
// are diag::ess_kernel as it is, applied to the draws, to c^2 and to the indicators 1[v <= q_p]
// (rankdiag::indicator_kernel as it is); this file has the steps that those do not have.
//
// x[m][s][q] and the J sequences of n draws are diag::Seqs; N = J n, draw i = j n + s in sequence order.
//
//   sort_kernel      the project's sorting kernel: a workgroup stages an [N_pad][TQ] fp64 tile of TQ columns in LDS
//                    (N_pad = the next power of two, TQ = tile_quantities(N): 128 KiB at most), sorts every column
//                    along N with a bitonic network, N_pad log2(N_pad) (log2(N_pad) + 1) / 4 compare-exchanges per column,
//                    and writes sorted[i][q].  Whether a column has a non-finite draw is decided on load, before the
//                    padding rows are filled with +inf: such a column is written as NaN, so a real +inf is never taken
//                    for padding.  Zeros are staged as +0.0.
//                    LDS layout: q is the fastest index of the tile AND of the thread numbering.  A compare-exchange
//                    step with distance j pairs row i (bit j clear) with row i + j; thread p takes column p % TQ of
//                    pair p / TQ, and consecutive pairs are consecutive rows within runs of j.  The 32 lanes that
//                    ds_read_b64 serves together therefore read runs of j TQ consecutive doubles: one whole 256-byte
//                    bank row without a conflict whenever j TQ >= 32, and runs separated by gaps of their own length,
//                    a 2-way conflict at worst, in the last few steps of every merge.  The walk along N with lane = row,
//                    at a stride of TQ doubles (32 lanes on 32 / TQ bank pairs: TQ-way, 32-way from TQ = 32 on), does
//                    not occur: no lane group ever strides along N.  Global loads and stores run along q as well.
//   moments_kernel   lane = quantity, thread group = one of the partial sums: the mean, then c = v - mean, m2, m4 and
//                    the c^2 array, two reads of the column
//   quantile_kernel  the type-7 quantile of one probability from two rows of the sorted array, in rankdiag's arithmetic
//   hdi_kernel       lane = quantity: the narrowest window of k + 1 consecutive order statistics, first minimum
//   mcse_kernel      mcse_mean and mcse_sd from the moments and the two ESS; the constant-column rule
//   mcse_quantile_kernel   lane = quantity: alpha, beta from ess_q, the inverse regularised incomplete beta function
//                    (num::beta_inverse) at Phi(-1) and Phi(1), the two ranks, and half the distance of their order
//                    statistics
//
// No atomics; every sum in an order fixed by N; a quantity's result is a function of its own column only, whatever the
// grid, the tile or the chunk.

namespace summary {

constexpr int kMaxDraws = SGMCMC_SUMMARY_MAX_DRAWS;           // N
constexpr int kMaxTile = SGMCMC_SUMMARY_MAX_TILE;             // TQ at most
constexpr int kWays = SGMCMC_DIAG_MEAN_WAYS;                  // partial sums of every sum over the draws
constexpr int kSortThreads = 1024;
constexpr int kThreads = 256;
constexpr int kMomentTile = kThreads / kWays;                 // quantities per workgroup of the moments pass
constexpr double kLowerTail = 0.1586553, kUpperTail = 0.8413447;      // Phi(-1), Phi(1) as posterior writes them
static_assert((kMaxDraws & (kMaxDraws - 1)) == 0 && (kMaxTile & (kMaxTile - 1)) == 0, "powers of two");
static_assert((size_t)kMaxDraws * sizeof(double) == 128 * 1024, "one column of the most draws is the whole tile");
static_assert((size_t)kMaxDraws * sizeof(double) + kMaxTile * sizeof(int) <= 160 * 1024, "LDS ceiling");

inline int padded(int N) {
  int p = 4;
  while (p < N) p <<= 1;
  return p;
}

// quantities per workgroup of the sort: the most columns of N_pad fp64 that fit 128 KiB, kMaxTile at most
inline int tile_quantities(int N) {
  if (N < 4 || N > kMaxDraws) return 0;
  const int t = kMaxDraws / padded(N);
  return t < kMaxTile ? t : kMaxTile;
}

inline bool make_seqs(int64_t chain_stride, int64_t draw_stride, int chains, int draws, int64_t quantities, int split,
                      diag::Seqs* A) {
  return diag::make_seqs(chain_stride, draw_stride, chains, draws, quantities, split, A) && A->J * A->n <= kMaxDraws;
}

__device__ __forceinline__ double plus_zero(double v) { return v == 0.0 ? 0.0 : v; }      // -0.0 is written as +0.0

template <typename T>
__global__ __launch_bounds__(kSortThreads) void sort_kernel(const T* __restrict__ x, diag::Seqs A, int64_t Q, int N,
                                                            int n_pad, int log_tq, double* __restrict__ sorted) {
  extern __shared__ __attribute__((aligned(16))) unsigned char summary_lds[];
  double* __restrict__ tile = reinterpret_cast<double*>(summary_lds);             // [n_pad][tq]
  const int tq = 1 << log_tq, cells = n_pad << log_tq;
  int* __restrict__ bad = reinterpret_cast<int*>(tile + cells);                   // [tq]: the column has a non-finite draw
  const int t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x << log_tq;

  if (t < tq) bad[t] = 0;
  __syncthreads();
  for (int e = t; e < cells; e += kSortThreads) {
    const int i = e >> log_tq, c = e & (tq - 1);
    double v = INFINITY;                          // padding: after every finite value
    if (i < N) {
      v = 0.0;                                    // a column past the end of the call: sorted, never stored
      if (q0 + c < Q) {
        const int j = i / A.n, s = i - j * A.n;
        v = plus_zero((double)x[diag::seq_offset(A, j) + (int64_t)s * A.draw_stride + q0 + c]);
        if (!num::is_finite(v)) bad[c] = 1;            // every writer stores the same value
      }
    }
    tile[e] = v;
  }

  num::bitonic_walk<false, kSortThreads>(tile, nullptr, n_pad, log_tq);        // written once, with the keyed sort's
  __syncthreads();

  for (int e = t; e < (N << log_tq); e += kSortThreads) {
    const int i = e >> log_tq, c = e & (tq - 1);
    if (q0 + c < Q) sorted[(int64_t)i * Q + q0 + c] = bad[c] ? NAN : tile[e];
  }
}

// draw i of the column at xq, in sequence order, widened
template <typename T>
__device__ __forceinline__ double draw(const T* __restrict__ xq, const diag::Seqs& A, int i) {
  const int j = i / A.n, s = i - j * A.n;
  return plus_zero((double)xq[diag::seq_offset(A, j) + (int64_t)s * A.draw_stride]);
}

// Every sum over the draws i = 0 .. N-1: kWays partial sums over i = r (mod kWays), each in ascending i from +0.0, the
// partials added in ascending r, every addition rounded once.  Thread group r of the workgroup forms partial r of the
// kMomentTile quantities (lane = quantity); the partials meet in LDS.
template <typename T>
__global__ __launch_bounds__(kThreads) void moments_kernel(const T* __restrict__ x, diag::Seqs A, int64_t Q,
                                                           double* __restrict__ mean_out, double* __restrict__ sd_out,
                                                           double* __restrict__ m2_out, double* __restrict__ m4_out,
                                                           double* __restrict__ csq) {
  __shared__ double part[3][kWays][kMomentTile];            // of sum v, sum c^2, sum c^4
  __shared__ int flags[kWays][kMomentTile];                 // bit 0: every draw is finite, bit 1: every draw equals the first
  const int lane = threadIdx.x % kMomentTile, way = threadIdx.x / kMomentTile;
  const int64_t q = (int64_t)blockIdx.x * kMomentTile + lane;
  const bool live = q < Q;
  const int N = A.J * A.n;
  const double Nd = (double)N;
  const T* __restrict__ xq = x + (live ? q : 0);
  const double first = live ? draw(xq, A, 0) : 0.0;

  double p = 0.0;
  bool finite = true, constant = true;
  if (live) {
    for (int i = way; i < N; i += kWays) {
      const double v = draw(xq, A, i);
      finite = finite && num::is_finite(v);
      constant = constant && v == first;
      p = __dadd_rn(p, v);
    }
  }
  part[0][way][lane] = p;
  flags[way][lane] = (finite ? 1 : 0) | (constant ? 2 : 0);
  __syncthreads();
  double sum = part[0][0][lane];
  int all = flags[0][lane];
#pragma unroll
  for (int r = 1; r < kWays; ++r) {
    sum = __dadd_rn(sum, part[0][r][lane]);
    all &= flags[r][lane];
  }
  finite = (all & 1) != 0;
  // a column whose draws are all equal has that value as its mean, whatever the sum of N copies rounds to
  const double mean = (all & 2) ? first : __ddiv_rn(sum, Nd);

  double p2 = 0.0, p4 = 0.0;
  if (live) {
    for (int i = way; i < N; i += kWays) {
      const double c = __dsub_rn(draw(xq, A, i), mean), c2 = __dmul_rn(c, c);
      csq[(int64_t)i * Q + q] = finite ? c2 : NAN;
      p2 = __dadd_rn(p2, c2);
      p4 = __dadd_rn(p4, __dmul_rn(c2, c2));
    }
  }
  part[1][way][lane] = p2;
  part[2][way][lane] = p4;
  __syncthreads();
  if (way != 0 || !live) return;
  double s2 = part[1][0][lane], s4 = part[2][0][lane];
#pragma unroll
  for (int r = 1; r < kWays; ++r) {
    s2 = __dadd_rn(s2, part[1][r][lane]);
    s4 = __dadd_rn(s4, part[2][r][lane]);
  }
  const double m2 = __ddiv_rn(s2, Nd), m4 = __ddiv_rn(s4, Nd);
  mean_out[q] = finite ? plus_zero(mean) : NAN;
  m2_out[q] = finite ? m2 : NAN;
  m4_out[q] = finite ? m4 : NAN;
  sd_out[q] = finite ? sqrt(__ddiv_rn(__dmul_rn(m2, Nd), __dsub_rn(Nd, 1.0))) : NAN;
}

// q_p from rows lo, hi of the sorted array: rankdiag::quantile_kernel's arithmetic (numpy's lerp, from the nearer
// neighbour), every operation rounded once
__global__ __launch_bounds__(kThreads) void quantile_kernel(const double* __restrict__ sorted, int lo, int hi,
                                                            double frac, int64_t Q, double* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= Q) return;
  const double a = sorted[(int64_t)lo * Q + q], b = sorted[(int64_t)hi * Q + q];
  const double d = __dsub_rn(b, a);
  out[q] = frac >= 0.5 ? __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, frac))) : __dadd_rn(a, __dmul_rn(d, frac));
}

__global__ __launch_bounds__(kThreads) void hdi_kernel(const double* __restrict__ sorted, int N, int k, int64_t Q,
                                                       double* __restrict__ lower, double* __restrict__ upper) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= Q) return;
  const double* __restrict__ col = sorted + q;
  int best = 0;
  double width = __dsub_rn(col[(int64_t)k * Q], col[0]);
  for (int i = 1; i + k < N; ++i) {
    const double w = __dsub_rn(col[(int64_t)(i + k) * Q], col[(int64_t)i * Q]);
    if (w < width) {                              // strict: the first window that attains the minimum
      width = w;
      best = i;
    }
  }
  lower[q] = col[(int64_t)best * Q];              // NaN rows (a non-finite draw) compare false throughout: NaN, NaN
  upper[q] = col[(int64_t)(best + k) * Q];
}

// ess_mean is read and, for a column without variance (m2 = 0), overwritten with NaN: the per-sequence means of
// sgmcmc_chain_ess may round away from a constant column's value and leave it a variance at rounding level
__global__ __launch_bounds__(kThreads) void mcse_kernel(const double* __restrict__ sd, const double* __restrict__ m2,
                                                        const double* __restrict__ m4, double* __restrict__ ess_mean,
                                                        const double* __restrict__ ess_sd, int64_t Q,
                                                        double* __restrict__ mcse_mean, double* __restrict__ mcse_sd) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= Q) return;
  const double v2 = m2[q], v4 = m4[q];
  const bool varies = v2 > 0.0;                   // false for NaN as well
  const double em = varies ? ess_mean[q] : NAN, es = varies ? ess_sd[q] : NAN;
  ess_mean[q] = em;
  mcse_mean[q] = __ddiv_rn(sd[q], sqrt(em));
  const double excess = __dsub_rn(v4, __dmul_rn(v2, v2));
  mcse_sd[q] = sqrt(__ddiv_rn(__ddiv_rn(__ddiv_rn(excess, es), v2), 4.0));
}

__global__ __launch_bounds__(kThreads) void mcse_quantile_kernel(const double* __restrict__ sorted, int N, double p,
                                                                 const double* __restrict__ ess_q, int64_t Q,
                                                                 double* __restrict__ mcse, double* __restrict__ a_out,
                                                                 double* __restrict__ b_out, int32_t* __restrict__ lo_out,
                                                                 int32_t* __restrict__ hi_out) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= Q) return;
  const double ess = ess_q[q], Nd = (double)N;
  double a = NAN, b = NAN, value = NAN;
  int lo = -1, hi = -1;
  if (ess > 0.0 && ess < INFINITY) {
    const double alpha = __dadd_rn(__dmul_rn(ess, p), 1.0), beta = __dadd_rn(__dmul_rn(ess, __dsub_rn(1.0, p)), 1.0);
    const num::Beta B = num::make_beta(alpha, beta);                             // alpha, beta >= 1 and finite
    a = num::beta_inverse(B, kLowerTail, -1.0);
    b = num::beta_inverse(B, kUpperTail, 1.0);
    if (a == a && b == b) {
      const double fl = floor(__dmul_rn(a, Nd)), ce = ceil(__dmul_rn(b, Nd));
      lo = min(max((int)fmax(fl, 1.0) - 1, 0), N - 1);                 // in range whatever the root search returned
      hi = min(max((int)fmin(ce, Nd) - 1, 0), N - 1);
      value = __ddiv_rn(__dsub_rn(sorted[(int64_t)hi * Q + q], sorted[(int64_t)lo * Q + q]), 2.0);
    }
  }
  mcse[q] = value;
  if (a_out) a_out[q] = a;
  if (b_out) b_out[q] = b;
  if (lo_out) lo_out[q] = lo;
  if (hi_out) hi_out[q] = hi;
}

inline bool grid_of(int64_t quantities, int per_block, dim3* grid) {
  const int64_t blocks = (quantities + per_block - 1) / per_block;
  if (blocks > 0x7fffffffll) return false;
  *grid = dim3((unsigned)blocks);
  return true;
}

}  // namespace summary

extern "C" int sgmcmc_summary_tile_quantities(int total_draws) { return summary::tile_quantities(total_draws); }

extern "C" int sgmcmc_summary_sort(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains,
                                   int draws, int64_t quantities, int split, double* sorted, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  if (!x || !sorted || !summary::make_seqs(chain_stride, draw_stride, chains, draws, quantities, split, &A))
    return (int)hipErrorInvalidValue;
  const int N = A.J * A.n, n_pad = summary::padded(N), tq = summary::tile_quantities(N);
  int log_tq = 0;
  while ((1 << log_tq) < tq) ++log_tq;
  dim3 grid;
  if (!summary::grid_of(quantities, tq, &grid)) return (int)hipErrorInvalidValue;
  static bool attr_done = false;
  if (!attr_done) {       // above 64 KiB of LDS per workgroup has to be asked for
    const int most = (int)((size_t)summary::kMaxDraws * sizeof(double) + summary::kMaxTile * sizeof(int));
    for (const void* k : {reinterpret_cast<const void*>(summary::sort_kernel<float>),
                          reinterpret_cast<const void*>(summary::sort_kernel<double>)}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, most);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  const size_t lds = (size_t)n_pad * tq * sizeof(double) + (size_t)tq * sizeof(int);
  const dim3 block(summary::kSortThreads);
  if (is_f64) SGMCMC_LAUNCH(summary::sort_kernel<double>, grid, block, lds, (hipStream_t)stream, (const double*)x, A,
                            quantities, N, n_pad, log_tq, sorted);
  else SGMCMC_LAUNCH(summary::sort_kernel<float>, grid, block, lds, (hipStream_t)stream, (const float*)x, A,
                     quantities, N, n_pad, log_tq, sorted);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_summary_moments(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains,
                                      int draws, int64_t quantities, int split, double* mean, double* sd, double* m2,
                                      double* m4, double* csq, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  dim3 grid;
  if (!x || !mean || !sd || !m2 || !m4 || !csq ||
      !summary::make_seqs(chain_stride, draw_stride, chains, draws, quantities, split, &A) ||
      !summary::grid_of(quantities, summary::kMomentTile, &grid))
    return (int)hipErrorInvalidValue;
  const dim3 block(summary::kThreads);
  if (is_f64) SGMCMC_LAUNCH(summary::moments_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x, A,
                            quantities, mean, sd, m2, m4, csq);
  else SGMCMC_LAUNCH(summary::moments_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, A,
                     quantities, mean, sd, m2, m4, csq);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_summary_quantile(const double* sorted, int chains, int draws, int split, double prob,
                                       int64_t quantities, double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  rankdiag::Stats S;
  dim3 grid;
  if (!sorted || !out || !summary::make_seqs(0, 0, chains, draws, quantities, split, &A) ||
      !rankdiag::make_stats(&prob, 1, A.J * A.n, &S) || !summary::grid_of(quantities, summary::kThreads, &grid))
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(summary::quantile_kernel, grid, dim3(summary::kThreads), 0, (hipStream_t)stream, sorted, S.lo[0],
                S.hi[0], S.frac[0], quantities, out);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_summary_hdi(const double* sorted, int chains, int draws, int split, double mass,
                                  int64_t quantities, double* lower, double* upper, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  dim3 grid;
  if (!sorted || !lower || !upper || !(mass > 0.0 && mass < 1.0) ||
      !summary::make_seqs(0, 0, chains, draws, quantities, split, &A) ||
      !summary::grid_of(quantities, summary::kThreads, &grid))
    return (int)hipErrorInvalidValue;
  const int N = A.J * A.n, k = (int)floor(mass * (double)N);
  if (k < 1 || k > N - 1) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(summary::hdi_kernel, grid, dim3(summary::kThreads), 0, (hipStream_t)stream, sorted, N, k, quantities,
                lower, upper);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_summary_mcse(const double* sd, const double* m2, const double* m4, double* ess_mean,
                                   const double* ess_sd, int64_t quantities, double* mcse_mean, double* mcse_sd,
                                   void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  dim3 grid;
  if (!sd || !m2 || !m4 || !ess_mean || !ess_sd || !mcse_mean || !mcse_sd || quantities <= 0 ||
      !summary::grid_of(quantities, summary::kThreads, &grid))
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(summary::mcse_kernel, grid, dim3(summary::kThreads), 0, (hipStream_t)stream, sd, m2, m4, ess_mean,
                ess_sd, quantities, mcse_mean, mcse_sd);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_summary_mcse_quantile(const double* sorted, int chains, int draws, int split, double prob,
                                            const double* ess_q, int64_t quantities, double* mcse, double* a, double* b,
                                            int32_t* lo, int32_t* hi, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  dim3 grid;
  if (!sorted || !ess_q || !mcse || !(prob > 0.0 && prob < 1.0) ||
      !summary::make_seqs(0, 0, chains, draws, quantities, split, &A) ||
      !summary::grid_of(quantities, summary::kThreads, &grid))
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(summary::mcse_quantile_kernel, grid, dim3(summary::kThreads), 0, (hipStream_t)stream, sorted,
                A.J * A.n, prob, ess_q, quantities, mcse, a, b, lo, hi);
  return (int)hipGetLastError();
}
