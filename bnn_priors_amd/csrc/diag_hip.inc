// Between-chain diagnostics of stored draws: split-R-hat and the effective sample size (Gelman et al., BDA3 section
// 11.4-11.5; Geyer 1992's initial positive / monotone sequence; Vehtari et al. 2021 WITHOUT the rank normalisation), on
// the device, in fp64, deterministic.  The reference has no such function: include/sgmcmc_hip.h states the definition.
//
// x[m][s][q]: M chains, S draws, Q quantities; q is the contiguous index (lane = quantity: coalesced loads), chains
// and draws have element strides.  Split: n = S / 2, sequence 2m = draws [0, n), 2m + 1 = draws [S - n, S) of chain
// m, J = 2M; else n = S, J = M.  Two kernels:
//
//   rhat_kernel  one thread per quantity streams its J sequences in order: the mean, then the centred sum of squares
//                (two reads of the data, no LDS)
//   ess_kernel   one workgroup per tile of kTile quantities walks the lags in blocks of kLagBlock.  Per block it goes
//                over the J sequences in order: stage the sequence's [n][kTile] tile in LDS, form the mean, centre in
//                place, accumulate the block's autocovariances (lane = quantity; each of the kGroups thread groups
//                owns kLagsPer consecutive lags and slides a register window over the column).  Then one thread per
//                quantity evaluates the block's Geyer pairs; the workgroup leaves when every quantity of the tile has
//                found its K.
//
// One arithmetic for both kernels (they agree bit for bit on R-hat), in an order fixed by (M, S, split) alone:
//   mean     kGroups partial sums over the draws s = r (mod kGroups), each in ascending s; the partials added in
//            ascending r; divided by n
//   a_j[t]   fma chain over s = 0 .. n-1-t of c_s c_{s+t}, divided by n; the sum over j in ascending j
//   mu_j     Welford's update over ascending j for var_j(mu_j)
// No atomics, no dependence on grid or tile: a quantity's result is a function of its own column only.

namespace diag {

constexpr int kMaxSeq = SGMCMC_DIAG_MAX_SEQ;         // n
constexpr int kMaxChains = SGMCMC_DIAG_MAX_CHAINS;   // J
constexpr int kLagBlock = SGMCMC_DIAG_LAG_BLOCK;
constexpr int kTile = SGMCMC_DIAG_TILE;              // quantities per workgroup of ess_kernel
constexpr int kThreads = 256;
constexpr int kGroups = kThreads / kTile;            // thread groups of ess_kernel = partial sums of every mean
constexpr int kLagsPer = kLagBlock / kGroups;        // consecutive lags per thread
static_assert(kTile == 32 && kGroups == SGMCMC_DIAG_MEAN_WAYS && kLagsPer * kGroups == kLagBlock && kLagBlock % 2 == 0, "diag geometry");
// the staged tile [n][kTile] fp64 (128 KiB at n = kMaxSeq) + partial sums + the block's mean autocovariances
constexpr size_t kSmallLds = (size_t)(kGroups + kLagBlock) * kTile * sizeof(double);
static_assert((size_t)kMaxSeq * kTile * sizeof(double) + kSmallLds + 64 <= 160 * 1024, "LDS ceiling");

struct Seqs {               // the J sequences of a call
  int64_t chain_stride, draw_stride;
  int draws, n, J, split;
};

__device__ __forceinline__ int64_t seq_offset(const Seqs& A, int j) {
  const int chain = A.split ? (j >> 1) : j;
  const int first = (A.split && (j & 1)) ? A.draws - A.n : 0;
  return (int64_t)chain * A.chain_stride + (int64_t)first * A.draw_stride;
}

struct Welford {            // running mean and sum of squared deviations of mu_0 .. mu_j
  double mean = 0.0, m2 = 0.0;
  __device__ __forceinline__ void push(double mu, int j) {
    const double d = mu - mean;
    mean = mean + d / (double)(j + 1);
    m2 = fma(d, mu - mean, m2);
  }
};

// W, var+ and R-hat from A0 = sum_j a_j[0] and the Welford state of the J means; false (and NaN) unless 0 < W < inf
__device__ __forceinline__ bool variances(double A0, const Welford& mu, int n, int J, double& W, double& varp,
                                          double& rhat) {
  const double nd = (double)n;
  W = (A0 / (double)J) * nd / (nd - 1.0);
  const double b_over_n = J > 1 ? mu.m2 / (double)(J - 1) : 0.0;
  varp = W * (nd - 1.0) / nd + b_over_n;
  const bool ok = W > 0.0 && W < INFINITY;
  rhat = ok ? sqrt(varp / W) : NAN;
  return ok;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void rhat_kernel(const T* __restrict__ x, Seqs A, int64_t Q,
                                                         double* __restrict__ rhat) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= Q) return;
  const int n = A.n;
  Welford mu;
  double A0 = 0.0;
  for (int j = 0; j < A.J; ++j) {
    const T* __restrict__ col = x + seq_offset(A, j) + q;
    double part[kGroups];
#pragma unroll
    for (int r = 0; r < kGroups; ++r) part[r] = 0.0;
    int s = 0;
    for (; s + kGroups <= n; s += kGroups) {
#pragma unroll
      for (int r = 0; r < kGroups; ++r) part[r] += (double)col[(int64_t)(s + r) * A.draw_stride];
    }
#pragma unroll
    for (int r = 0; r < kGroups; ++r)
      if (s + r < n) part[r] += (double)col[(int64_t)(s + r) * A.draw_stride];
    double sum = part[0];
#pragma unroll
    for (int r = 1; r < kGroups; ++r) sum += part[r];
    const double mean = sum / (double)n;
    double ss = 0.0;
    for (s = 0; s < n; ++s) {
      const double c = (double)col[(int64_t)s * A.draw_stride] - mean;
      ss = fma(c, c, ss);
    }
    A0 += ss / (double)n;
    mu.push(mean, j);
  }
  double W, varp, r;
  variances(A0, mu, n, A.J, W, varp, r);
  rhat[q] = r;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void ess_kernel(const T* __restrict__ x, Seqs A, int64_t Q,
                                                        double* __restrict__ ess, double* __restrict__ rhat,
                                                        int32_t* __restrict__ pairs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char diag_lds[];
  double* __restrict__ tile = reinterpret_cast<double*>(diag_lds);          // [n][kTile], centred
  double* __restrict__ part = tile + (size_t)A.n * kTile;                   // [kGroups][kTile]
  double* __restrict__ acov = part + kGroups * kTile;                       // [kLagBlock][kTile]: mean_j a_j[t]
  int* __restrict__ vote = reinterpret_cast<int*>(acov + kLagBlock * kTile);

  const int t = threadIdx.x, lane = t % kTile, grp = t / kTile;
  const int64_t q = (int64_t)blockIdx.x * kTile + lane;
  const bool live = q < Q;
  const int n = A.n, J = A.J, half = n / 2;
  const double nd = (double)n;

  // state of the quantity's evaluating thread (grp == 0)
  Welford mu;
  double W = 0.0, varp = 0.0, r_hat = NAN, p_mono = 0.0, p_sum = 0.0;
  int K = 0;
  bool done = !live;

  // Lags beyond a quantity's 2K + 1 enter nothing (tau sums P'_k for k < K only, and K is fixed by P_1 .. P_K), so
  // leaving once every quantity of the tile has its K cannot change a result: a quantity that is done ignores every
  // later block.
  for (int t0 = 0; t0 < 2 * half; t0 += kLagBlock) {
    const int lag0 = t0 + grp * kLagsPer;         // this thread's lags: lag0 .. lag0 + kLagsPer - 1
    double tot[kLagsPer];
#pragma unroll
    for (int i = 0; i < kLagsPer; ++i) tot[i] = 0.0;

    for (int j = 0; j < J; ++j) {
      const T* __restrict__ col = x + seq_offset(A, j) + q;
      __syncthreads();                            // the previous sequence's tile and partials have been read
      double p = 0.0;
      for (int s = grp; s < n; s += kGroups) {
        const double v = live ? (double)col[(int64_t)s * A.draw_stride] : 0.0;
        tile[s * kTile + lane] = v;
        p += v;
      }
      part[grp * kTile + lane] = p;
      __syncthreads();
      double sum = part[lane];
#pragma unroll
      for (int r = 1; r < kGroups; ++r) sum += part[r * kTile + lane];
      const double mean = sum / nd;
      for (int s = grp; s < n; s += kGroups) tile[s * kTile + lane] -= mean;
      if (t0 == 0 && grp == 0) mu.push(mean, j);
      __syncthreads();

      // a_j[lag0 + i] = (1/n) sum_s c_s c_{s + lag0 + i}: w[i] slides over c_{s + lag0 + i}; past the end of the
      // sequence the window holds zeros, whose products leave the sums as they are
      double a[kLagsPer], w[kLagsPer];
#pragma unroll
      for (int i = 0; i < kLagsPer; ++i) {
        a[i] = 0.0;
        w[i] = lag0 + i < n ? tile[(lag0 + i) * kTile + lane] : 0.0;
      }
      const int terms = n - lag0;                 // of the longest of this thread's sums
#pragma unroll 4
      for (int s = 0; s < terms; ++s) {
        const double c = tile[s * kTile + lane];
        const int nxt = s + lag0 + kLagsPer;
        const double in = nxt < n ? tile[nxt * kTile + lane] : 0.0;
#pragma unroll
        for (int i = 0; i < kLagsPer; ++i) a[i] = fma(c, w[i], a[i]);
#pragma unroll
        for (int i = 0; i + 1 < kLagsPer; ++i) w[i] = w[i + 1];
        w[kLagsPer - 1] = in;
      }
#pragma unroll
      for (int i = 0; i < kLagsPer; ++i) tot[i] += a[i] / nd;
    }

    if (t == 0) *vote = 0;
#pragma unroll
    for (int i = 0; i < kLagsPer; ++i) acov[(grp * kLagsPer + i) * kTile + lane] = tot[i];   // sum_j a_j[t]
    __syncthreads();
    if (grp == 0 && !done) {
      if (t0 == 0 && !variances(acov[lane], mu, n, J, W, varp, r_hat)) done = true;           // NaN rule: K stays 0
      const int k_end = min((t0 + kLagBlock) / 2, half);
      for (int k = t0 / 2; k < k_end && !done; ++k) {
        const double m0 = acov[(2 * k - t0) * kTile + lane] / (double)J;
        const double m1 = acov[(2 * k + 1 - t0) * kTile + lane] / (double)J;
        const double rho0 = k == 0 ? 1.0 : 1.0 - (W - m0) / varp;
        const double rho1 = 1.0 - (W - m1) / varp;
        const double P = rho0 + rho1;
        if (k >= 1 && P <= 0.0) {
          K = k;
          done = true;
        } else {
          p_mono = k == 0 ? P : fmin(p_mono, P);
          p_sum += p_mono;
        }
      }
      if (!done && k_end == half) {
        K = half;
        done = true;
      }
      if (!done) *vote = 1;                       // every writer stores the same value
    }
    __syncthreads();
    const int more = *vote;
    if (!more) break;
  }

  if (grp == 0 && live) {
    const bool ok = r_hat == r_hat;               // variances() gave a number
    const double total = (double)J * nd;
    double tau = -1.0 + 2.0 * p_sum;
    const double floor_tau = 1.0 / log10(total);
    if (tau < floor_tau) tau = floor_tau;
    ess[q] = ok ? total / tau : NAN;
    if (rhat) rhat[q] = r_hat;
    if (pairs) pairs[q] = K;
  }
}

inline bool make_seqs(int64_t chain_stride, int64_t draw_stride, int chains, int draws, int64_t quantities, int split,
                      Seqs* A) {
  if (chains <= 0 || draws <= 0 || quantities <= 0 || chain_stride < 0 || draw_stride < 0) return false;
  const int n = split ? draws / 2 : draws;
  const int64_t J = split ? 2 * (int64_t)chains : chains;
  if (n < 4 || n > kMaxSeq || J > kMaxChains) return false;
  *A = Seqs{chain_stride, draw_stride, draws, n, (int)J, split ? 1 : 0};
  return true;
}

}  // namespace diag

extern "C" int sgmcmc_chain_rhat(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains,
                                 int draws, int64_t quantities, int split, double* rhat, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  if (!x || !rhat || !diag::make_seqs(chain_stride, draw_stride, chains, draws, quantities, split, &A))
    return (int)hipErrorInvalidValue;
  const int64_t blocks = (quantities + diag::kThreads - 1) / diag::kThreads;
  if (blocks > 0x7fffffffll) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(diag::kThreads);
  if (is_f64) SGMCMC_LAUNCH(diag::rhat_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x, A,
                            quantities, rhat);
  else SGMCMC_LAUNCH(diag::rhat_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, A, quantities,
                     rhat);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_chain_ess(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains,
                                int draws, int64_t quantities, int split, double* ess, double* rhat, int32_t* pairs,
                                void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  diag::Seqs A;
  if (!x || !ess || !diag::make_seqs(chain_stride, draw_stride, chains, draws, quantities, split, &A))
    return (int)hipErrorInvalidValue;
  const int64_t blocks = (quantities + diag::kTile - 1) / diag::kTile;
  if (blocks > 0x7fffffffll) return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)A.n * diag::kTile * sizeof(double) + diag::kSmallLds + 16;
  static bool attr_done = false;
  if (!attr_done) {       // above 64 KiB of LDS per workgroup has to be asked for
    const int most = (int)((size_t)diag::kMaxSeq * diag::kTile * sizeof(double) + diag::kSmallLds + 16);
    for (const void* k : {reinterpret_cast<const void*>(diag::ess_kernel<float>),
                          reinterpret_cast<const void*>(diag::ess_kernel<double>)}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, most);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  const dim3 grid((unsigned)blocks), block(diag::kThreads);
  if (is_f64) SGMCMC_LAUNCH(diag::ess_kernel<double>, grid, block, lds, (hipStream_t)stream, (const double*)x, A,
                            quantities, ess, rhat, pairs);
  else SGMCMC_LAUNCH(diag::ess_kernel<float>, grid, block, lds, (hipStream_t)stream, (const float*)x, A, quantities,
                     ess, rhat, pairs);
  return (int)hipGetLastError();
}
