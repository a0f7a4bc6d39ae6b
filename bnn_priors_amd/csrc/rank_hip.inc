// Rank-normalised R-hat with bulk and tail ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021): the steps that
// diag_hip.inc does not have -- average ranks and their normal scores, the order statistics behind the median and the
// tail quantiles, and the tail indicators.  The R-hat and ESS of the resulting [J][n][Q] arrays are diag::rhat_kernel
// and diag::ess_kernel as they are.  include/sgmcmc_hip.h states the definition.
//
// x[m][s][q] and the J sequences of n draws are diag::Seqs; N = J n, draw i = j n + s in sequence order.
//
//   score_kernel      lane = quantity (coalesced loads of a draw's row), a thread owns kOwn consecutive draws of its
//                     quantity in registers and streams all N draws of the column, counting for each of its own draws
//                     how many are less and how many are equal (fp64 compares: -0.0 = 0.0), and noting a non-finite
//                     value.  A workgroup is kLanes quantities x kWaves own-blocks; blockIdx.y covers the rest.  The
//                     column is re-read N / kOwn times, out of L2; the kernel is bound by its N^2 Q comparisons.  Then
//                     z = ndtri((less + (equal + 1) / 2 - 3/8) / (N + 1/4)) for the own draws, and an own draw that
//                     covers a requested order-statistic position k (less <= k < less + equal) stores its value: every
//                     thread that qualifies stores the same bits (zeros are stored as +0.0).  With a centre the draws
//                     are folded on load: |x - centre|, the subtraction rounded once.
//   quantile_kernel   q_p = v_(lo) + (v_(hi) - v_(lo)) frac per quantity, from frac = 0.5 on in the form
//                     v_(hi) - (v_(hi) - v_(lo)) (1 - frac) (numpy's arithmetic); every operation rounded once
//   indicator_kernel  1[x <= q] as fp32, for two quantiles at once
//
// No LDS, no cross-thread step, no atomics: ranks are integer counts, and a quantity's result is a function of its own
// column only, whatever the grid or the chunk.  A column with a non-finite draw gets NaN for every z and every order
// statistic (hence NaN quantiles, constant indicators and NaN everywhere downstream).

namespace rankdiag {

constexpr int kOwn = SGMCMC_RANK_OWN;        // draws a thread ranks
constexpr int kLanes = 64;                   // quantities per workgroup: one per lane of a wave
constexpr int kWaves = 4;                    // own-blocks per workgroup
constexpr int kThreads = kLanes * kWaves;
constexpr int kMaxProbs = SGMCMC_RANK_MAX_PROBS;
static_assert((int64_t)diag::kMaxSeq * diag::kMaxChains <= 0x7fffffffll / 2, "the counts fit int32");

struct Stats {              // the order statistics a score pass stores: positions lo[i], hi[i] -> rows 2 i, 2 i + 1
  int count;
  int lo[kMaxProbs], hi[kMaxProbs];
  double frac[kMaxProbs];
};

// pos = (N - 1) p, lo = floor(pos), hi = min(lo + 1, N - 1), frac = pos - lo; each operation rounded once
inline bool make_stats(const double* probs, int nprobs, int N, Stats* S) {
  if (nprobs < 0 || nprobs > kMaxProbs || (nprobs > 0 && !probs)) return false;
  S->count = nprobs;
  for (int i = 0; i < kMaxProbs; ++i) {
    S->lo[i] = S->hi[i] = 0;
    S->frac[i] = 0.0;
  }
  for (int i = 0; i < nprobs; ++i) {
    const double p = probs[i];
    if (!(p > 0.0 && p < 1.0)) return false;
    const double pos = (double)(N - 1) * p;
    const int lo = (int)floor(pos);
    S->lo[i] = lo;
    S->hi[i] = lo + 1 < N - 1 ? lo + 1 : N - 1;
    S->frac[i] = pos - (double)lo;
  }
  return true;
}

// the value that is ranked: the draw widened, or folded about the quantity's centre
template <typename T>
__device__ __forceinline__ double ranked(T raw, bool fold, double centre) {
  const double v = (double)raw;
  return fold ? fabs(__dsub_rn(v, centre)) : v;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void score_kernel(const T* __restrict__ x, diag::Seqs A, int64_t Q,
                                                          const double* __restrict__ centre, Stats S,
                                                          double* __restrict__ z, double* __restrict__ ostat) {
  const int lane = threadIdx.x % kLanes, wave = threadIdx.x / kLanes;
  const int64_t q = (int64_t)blockIdx.x * kLanes + lane;
  const int n = A.n, J = A.J, N = J * n;
  const int first = ((int)blockIdx.y * kWaves + wave) * kOwn;       // this thread's draws: first .. first + kOwn - 1
  if (q >= Q || first >= N) return;
  const bool fold = centre != nullptr;
  const double c = fold ? centre[q] : 0.0;

  double own[kOwn];
  int less[kOwn], equal[kOwn];
#pragma unroll
  for (int r = 0; r < kOwn; ++r) {
    const int i = min(first + r, N - 1);          // past the end: a copy of the last draw, which stores nothing
    const int j = i / n, s = i - j * n;
    own[r] = ranked(x[diag::seq_offset(A, j) + (int64_t)s * A.draw_stride + q], fold, c);
    less[r] = 0;
    equal[r] = 0;
  }

  bool finite = true;
  for (int j = 0; j < J; ++j) {
    const T* __restrict__ col = x + diag::seq_offset(A, j) + q;
#pragma unroll 4
    for (int s = 0; s < n; ++s) {
      const double v = ranked(col[(int64_t)s * A.draw_stride], fold, c);
      finite = finite && fabs(v) < INFINITY;      // false for NaN as well
#pragma unroll
      for (int r = 0; r < kOwn; ++r) {
        less[r] += v < own[r];
        equal[r] += v == own[r];
      }
    }
  }

  const double denom = (double)N + 0.25;
#pragma unroll
  for (int r = 0; r < kOwn; ++r) {
    const int i = first + r;
    if (i >= N) continue;
    // the average rank less + (equal + 1) / 2 and its numerator are exact; the quotient is one rounded division
    const double numer = (double)less[r] + 0.5 * (double)(equal[r] + 1) - 0.375;
    z[(int64_t)i * Q + q] = finite ? num::ndtri(numer / denom) : NAN;
    if (ostat && finite) {
      const double v = own[r] == 0.0 ? 0.0 : own[r];      // -0.0 is written as +0.0
      for (int k = 0; k < S.count; ++k) {
        if (less[r] <= S.lo[k] && S.lo[k] < less[r] + equal[r]) ostat[(int64_t)(2 * k) * Q + q] = v;
        if (less[r] <= S.hi[k] && S.hi[k] < less[r] + equal[r]) ostat[(int64_t)(2 * k + 1) * Q + q] = v;
      }
    }
  }
  if (ostat && !finite && first == 0)
    for (int k = 0; k < 2 * S.count; ++k) ostat[(int64_t)k * Q + q] = NAN;
}

__global__ __launch_bounds__(256) void quantile_kernel(const double* __restrict__ ostat, Stats S, int64_t Q,
                                                       double* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  for (int k = 0; k < S.count; ++k) {
    const double lo = ostat[(int64_t)(2 * k) * Q + q], hi = ostat[(int64_t)(2 * k + 1) * Q + q];
    const double d = __dsub_rn(hi, lo), t = S.frac[k];       // numpy's lerp: from the nearer neighbour
    out[(int64_t)k * Q + q] = t >= 0.5 ? __dsub_rn(hi, __dmul_rn(d, __dsub_rn(1.0, t))) : __dadd_rn(lo, __dmul_rn(d, t));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void indicator_kernel(const T* __restrict__ x, diag::Seqs A, int64_t Q,
                                                        const double* __restrict__ q_lower,
                                                        const double* __restrict__ q_upper,
                                                        float* __restrict__ lower, float* __restrict__ upper) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (q >= Q) return;
  const double ql = q_lower[q], qu = q_upper[q];
  const T* __restrict__ col = x + diag::seq_offset(A, j) + q;
  const int64_t out0 = (int64_t)j * A.n * Q + q;
  for (int s = 0; s < A.n; ++s) {
    const double v = (double)col[(int64_t)s * A.draw_stride];
    lower[out0 + (int64_t)s * Q] = v <= ql ? 1.0f : 0.0f;
    upper[out0 + (int64_t)s * Q] = v <= qu ? 1.0f : 0.0f;
  }
}

}  // namespace rankdiag

extern "C" int sgmcmc_chain_rank_scores(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride,
                                        int chains, int draws, int64_t quantities, int split, const double* centre,
                                        const double* probs, int nprobs, double* z, double* ostat, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  rankdiag::Stats S;
  if (!x || !z || !diag::make_seqs(chain_stride, draw_stride, chains, draws, quantities, split, &A) ||
      !rankdiag::make_stats(probs, nprobs, A.J * A.n, &S) || (nprobs > 0 && !ostat))
    return (int)hipErrorInvalidValue;
  const int64_t blocks = (quantities + rankdiag::kLanes - 1) / rankdiag::kLanes;
  if (blocks > 0x7fffffffll) return (int)hipErrorInvalidValue;
  const int per_group = rankdiag::kOwn * rankdiag::kWaves;
  const dim3 grid((unsigned)blocks, (unsigned)((A.J * A.n + per_group - 1) / per_group)), block(rankdiag::kThreads);
  double* stats_out = nprobs > 0 ? ostat : nullptr;
  if (is_f64) SGMCMC_LAUNCH(rankdiag::score_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x, A,
                            quantities, centre, S, z, stats_out);
  else SGMCMC_LAUNCH(rankdiag::score_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, A,
                     quantities, centre, S, z, stats_out);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_chain_quantiles(const double* ostat, int chains, int draws, int split, const double* probs,
                                      int nprobs, int64_t quantities, double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  rankdiag::Stats S;
  if (!ostat || !out || nprobs < 1 || !diag::make_seqs(0, 0, chains, draws, quantities, split, &A) ||
      !rankdiag::make_stats(probs, nprobs, A.J * A.n, &S))
    return (int)hipErrorInvalidValue;
  const int64_t blocks = (quantities + 255) / 256;
  if (blocks > 0x7fffffffll) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(rankdiag::quantile_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ostat, S,
                quantities, out);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_chain_tail_indicators(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride,
                                            int chains, int draws, int64_t quantities, int split,
                                            const double* q_lower, const double* q_upper, float* lower, float* upper,
                                            void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  if (!x || !q_lower || !q_upper || !lower || !upper ||
      !diag::make_seqs(chain_stride, draw_stride, chains, draws, quantities, split, &A))
    return (int)hipErrorInvalidValue;
  const int64_t blocks = (quantities + 255) / 256;
  if (blocks > 0x7fffffffll) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks, (unsigned)A.J), block(256);
  if (is_f64) SGMCMC_LAUNCH(rankdiag::indicator_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x,
                            A, quantities, q_lower, q_upper, lower, upper);
  else SGMCMC_LAUNCH(rankdiag::indicator_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, A,
                     quantities, q_lower, q_upper, lower, upper);
  return (int)hipGetLastError();
}
