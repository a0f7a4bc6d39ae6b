// Calibration and out-of-distribution metrics of a posterior ensemble (reference: bnn_priors/exp_utils.py:300-380,
// bnn_priors/third_party/calibration_error.py): everything after the per-sample predictive tables, on the device, in
// fp64, deterministic.  Four kernels:
//
//   ensemble_kernel  lme = logsumexp_e acc[e, n, :] - log E, probs = softmax(lme), the row's max-prob / first argmax /
//                    hit: the one pass over the [E, N, C] table, one thread per (row, class) so that a block reads
//                    consecutive rows of each sample's [N, C] plane
//   order_kernel     np.argsort(kind="stable") of independent fp64 columns by counting:
//                    rank_i = #{j : a_j < a_i} + #{j < i : a_j == a_i}, keys staged tile by tile in LDS, perm[rank_i] = i.
//                    Keys compare as numpy orders them: -0.0 == 0.0, subnormals exact, NaN after everything (ties by index)
//   calib_kernel     one workgroup per sorted column: the `> 0` filter, even or adaptive bin bounds, per-bin integer
//                    count / integer hits / fp64 score sum over the bin's contiguous range of the sorted column, and the
//                    reference's weighted error (eps in the weight, weights over bins)
//   rank_kernel      one workgroup: integer cumulative TP / FP at every distinct threshold, the ROC trapezoids in
//                    integers and average precision as a fixed-order fp64 sum
//
// Every sum runs in an order fixed by the sizes alone; integer quantities are exact.  No atomics, no host round trip.

namespace calib {

constexpr int kMaxClasses = 128;
constexpr int kMaxRows = 131072;
constexpr int kMaxBins = 4096;
constexpr double kEps = 2.220446049250313e-16;   // np.finfo(np.float64).eps = 2^-52

__global__ __launch_bounds__(256) void ensemble_kernel(const double* __restrict__ acc, const int64_t* __restrict__ labels,
                                                       int E, int N, int C, double* __restrict__ probs,
                                                       double* __restrict__ conf, int64_t* __restrict__ pred,
                                                       int64_t* __restrict__ hit) {
  __shared__ double row[256];
  const int rows = 256 / C;                       // >= 2 rows per block (C <= 128)
  const int t = threadIdx.x, r = t / C, c = t - r * C;
  const int64_t n0 = (int64_t)blockIdx.x * rows;
  if (r < rows && n0 + r < N) {
    const size_t plane = (size_t)N * C;
    const double* __restrict__ a = acc + (size_t)(n0 + r) * C + c;
    double m = -INFINITY, s = 0.0;
    int e = 0;
    for (; e + 4 <= E; e += 4)
      num::lse_add4(m, s, a[(size_t)e * plane], a[(size_t)(e + 1) * plane], a[(size_t)(e + 2) * plane],
                    a[(size_t)(e + 3) * plane]);
    for (; e < E; ++e) num::lse_add1(m, s, a[(size_t)e * plane]);
    row[t] = num::lse_log_mean(m, s, E);
  }
  __syncthreads();
  const int64_t n = n0 + t;
  if (t < rows && n < N) {
    double* l = row + t * C;
    num::row_softmax(l, C, probs + n * C);
    num::row_max(l, C, n, labels, conf, pred, hit);
  }
}

__global__ __launch_bounds__(256) void row_max_kernel(const double* __restrict__ probs, const int64_t* __restrict__ labels,
                                                      int N, int C, double* __restrict__ conf,
                                                      int64_t* __restrict__ pred, int64_t* __restrict__ hit) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n < N) num::row_max(probs + n * C, C, n, labels, conf, pred, hit);
}

// fp64 -> uint64 with the same order as numpy's sort: -0.0 and 0.0 equal, NaN (any payload) last
__device__ __forceinline__ uint64_t order_key(double x) {
  if (x != x) return ~0ull;
  if (x == 0.0) return 0x8000000000000000ull;
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

constexpr int kOrderPer = 4;    // keys per thread: each LDS read of the tile serves four comparisons

__global__ __launch_bounds__(256) void order_kernel(const double* __restrict__ keys, int64_t elem_stride,
                                                    int64_t col_stride, int n, int32_t* __restrict__ perm) {
  __shared__ uint64_t tile[256];
  const int t = threadIdx.x, col = blockIdx.y;
  const double* __restrict__ kc = keys + (int64_t)col * col_stride;
  int idx[kOrderPer], rank[kOrderPer];
  uint64_t key[kOrderPer];
#pragma unroll
  for (int k = 0; k < kOrderPer; ++k) {
    idx[k] = blockIdx.x * (256 * kOrderPer) + k * 256 + t;
    key[k] = idx[k] < n ? order_key(kc[(int64_t)idx[k] * elem_stride]) : 0;
    rank[k] = 0;
  }
  for (int base = 0; base < n; base += 256) {
    const int cnt = min(256, n - base);
    __syncthreads();
    if (t < cnt) tile[t] = order_key(kc[(int64_t)(base + t) * elem_stride]);
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const uint64_t kj = tile[j];
      const int jg = base + j;
#pragma unroll
      for (int k = 0; k < kOrderPer; ++k) rank[k] += (kj < key[k]) | ((kj == key[k]) & (jg < idx[k]));
    }
  }
  int32_t* __restrict__ pc = perm + (int64_t)col * n;
#pragma unroll
  for (int k = 0; k < kOrderPer; ++k)
    if (idx[k] < n) pc[rank[k]] = idx[k];         // ranks of a column are a permutation of 0..n-1
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int wave_sum_int(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// bounds != NULL: the n_bounds even upper bounds; else adaptive with n_bounds = B bins (B - 1 upper bounds)
__global__ __launch_bounds__(256) void calib_kernel(const double* __restrict__ keys, int64_t elem_stride,
                                                    int64_t col_stride, const int32_t* __restrict__ perm,
                                                    const int64_t* __restrict__ target, int class_conditional, int n,
                                                    const double* __restrict__ bounds, int n_bounds, int l2,
                                                    double* __restrict__ col_err) {
  __shared__ int hi_pos[kMaxBins + 1];
  __shared__ double term[kMaxBins + 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, col = blockIdx.x;
  const double* __restrict__ kc = keys + (int64_t)col * col_stride;
  const int32_t* __restrict__ pc = perm + (int64_t)col * n;
  const int64_t positive = class_conditional ? col : 1;
  auto row_at = [&](int q) { return min(max(pc[q], 0), n - 1); };
  auto sorted = [&](int q) { return kc[(int64_t)row_at(q) * elem_stride]; };

  const double last = sorted(n - 1);
  if (last != last) {                              // NaN sorts last: the column holds one
    if (t == 0) col_err[col] = last;
    return;
  }
  // drop keys that are not > 0: they are a prefix of the sorted column
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted(mid) > 0.0) hi = mid; else lo = mid + 1;
  }
  const int p0 = lo, n_eff = n - p0;
  if (n_eff == 0) {
    if (t == 0) col_err[col] = 0.0;
    return;
  }
  const int nb = bounds ? n_bounds : max(n_bounds - 1, 0);
  const double step = (double)n_eff / (double)n_bounds;        // np.linspace(0, n, B, endpoint=False)
  for (int k = t; k < nb; k += 256) {
    const double edge = bounds ? bounds[k] : sorted(p0 + min((int)rint((double)(k + 1) * step), n_eff - 1));
    int a = p0, b = n;                             // np.digitize: bin k holds bound[k-1] <= x < bound[k]
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (sorted(mid) < edge) a = mid + 1; else b = mid;
    }
    hi_pos[k] = a;
  }
  if (t == 0) hi_pos[nb] = n;
  __syncthreads();
  for (int k = wave; k <= nb; k += 4) {
    const int b0 = k ? hi_pos[k - 1] : p0, b1 = hi_pos[k];
    double S = 0.0;
    int H = 0;
    for (int q = b0 + lane; q < b1; q += 64) {
      const int r = row_at(q);
      S += kc[(int64_t)r * elem_stride];
      H += target[r] == positive;
    }
    S = wave_sum(S);
    H = wave_sum_int(H);
    if (lane == 0) {
      const double cnt = (double)(b1 - b0) + kEps;
      const double err = ((double)H / cnt - S / cnt) * (cnt / (double)n_eff);
      term[k] = l2 ? err * err : fabs(err);
    }
  }
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int k = 0; k <= nb; ++k) sum += term[k];
    col_err[col] = sum;
  }
}

// calibration_error.py:257-277: sum_j err_j / C over the classes of a class-conditional metric, sqrt for l2
__global__ void calib_combine_kernel(const double* __restrict__ col_err, int ncols, int class_conditional, int l2,
                                     double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double e = col_err[0];
  if (class_conditional) {
    e = 0.0;
    for (int j = 0; j < ncols; ++j) e += col_err[j] / (double)ncols;
  }
  out[0] = l2 ? sqrt(e) : e;
}

constexpr int kRankThreads = 1024;
constexpr int kNone = 0x7fffffff;

// rows [0, n_pos) of scores are the positives (in-distribution), [n_pos, n) the negatives; perm: their ascending
// stable order.  out[0] = AUROC, out[1] = average precision, out[2] = 1 if a score is NaN (then out[0..1] = NaN)
__global__ __launch_bounds__(kRankThreads) void rank_kernel(const double* __restrict__ scores,
                                                            const int32_t* __restrict__ perm, int n, int n_pos,
                                                            double* __restrict__ out) {
  __shared__ int incl[kRankThreads], before[kRankThreads], sfx[kRankThreads];
  __shared__ long long area_s[kRankThreads];
  __shared__ double ap_s[kRankThreads];
  const int t = threadIdx.x;
  auto row_at = [&](int q) { return min(max(perm[q], 0), n - 1); };
  auto sorted = [&](int q) { return scores[row_at(q)]; };
  const double last = sorted(n - 1);
  if (last != last) {
    if (t == 0) { out[0] = last; out[1] = last; out[2] = 1.0; }
    return;
  }
  // thread t owns the ascending positions [q0, q1); a group of tied scores starts where the value changes
  const int L = (n + kRankThreads - 1) / kRankThreads;
  const int q0 = min(t * L, n), q1 = min(q0 + L, n);
  int pos = 0, fs = kNone, pb = 0;              // positives in the chunk; its first group start, positives before it
  for (int q = q0; q < q1; ++q) {
    if (fs == kNone && (q == 0 || sorted(q) != sorted(q - 1))) { fs = q; pb = pos; }
    pos += row_at(q) < n_pos;
  }
  incl[t] = pos;
  before[t] = pb;
  sfx[t] = fs;
  __syncthreads();
  num::block_scan<int, num::Add, false, kRankThreads>(incl, num::Add());     // incl[t] = #positives at positions < q1
  num::block_scan<int, num::Min, true, kRankThreads>(sfx, num::Min());      // sfx[t] = the first group start in chunks >= t
  const int nxt = t + 1 < kRankThreads ? sfx[t + 1] : kNone;
  // walk the chunk downwards: a group [q, e) with e the next start above it.  prefix(x) = #positives below x,
  // tp(x) = P - prefix(x), fp(x) = (n - x) - tp(x): the cumulative counts at the threshold sorted(x), from the top
  const long long P = n_pos, Nn = (long long)n - n_pos;
  int e = n;
  long long pe = P;
  if (nxt != kNone) {
    e = nxt;
    const int owner = e / L;
    pe = (owner ? incl[owner - 1] : 0) + before[owner];
  }
  long long pq = incl[t], area2 = 0;
  double ap = 0.0;
  double v_hi = q1 > q0 ? sorted(q1 - 1) : 0.0;
  for (int q = q1 - 1; q >= q0; --q) {
    pq -= row_at(q) < n_pos;
    const double v_lo = q > 0 ? sorted(q - 1) : 0.0;
    if (q == 0 || v_hi != v_lo) {
      const long long tp = P - pq, fp = ((long long)n - q) - tp, tp_prev = P - pe, fp_prev = ((long long)n - e) - tp_prev;
      area2 += (fp - fp_prev) * (tp + tp_prev);
      ap += ((double)tp / (double)P - (double)tp_prev / (double)P) * ((double)tp / (double)(tp + fp));
      e = q;
      pe = pq;
    }
    v_hi = v_lo;
  }
  area_s[t] = area2;
  ap_s[t] = ap;
  __syncthreads();
  for (int half = kRankThreads / 2; half > 0; half >>= 1) {
    if (t < half) { area_s[t] += area_s[t + half]; ap_s[t] += ap_s[t + half]; }
    __syncthreads();
  }
  if (t == 0) {
    out[0] = (double)area_s[0] / (2.0 * (double)P * (double)Nn);
    out[1] = ap_s[0];
    out[2] = 0.0;
  }
}

}  // namespace calib

extern "C" int sgmcmc_ensemble_probs(const double* acc, const int64_t* labels, int samples, int rows, int classes,
                                     double* probs, double* conf, int64_t* pred, int64_t* hit, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!acc || !probs || !conf || !pred || (labels != nullptr) != (hit != nullptr) || samples <= 0 || rows <= 0 ||
      classes <= 0 || classes > calib::kMaxClasses)
    return (int)hipErrorInvalidValue;
  const int per = 256 / classes;
  SGMCMC_LAUNCH(calib::ensemble_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(256), 0, (hipStream_t)stream,
                acc, labels, samples, rows, classes, probs, conf, pred, hit);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_row_max(const double* probs, const int64_t* labels, int rows, int classes, double* conf,
                              int64_t* pred, int64_t* hit, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!probs || !conf || !pred || (labels != nullptr) != (hit != nullptr) || rows <= 0 || classes <= 0 ||
      classes > calib::kMaxClasses)
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(calib::row_max_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                probs, labels, rows, classes, conf, pred, hit);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_stable_order(const double* keys, int64_t elem_stride, int64_t col_stride, int n, int ncols,
                                   int32_t* perm, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!keys || !perm || n <= 0 || n > calib::kMaxRows || ncols <= 0 || ncols > 65535 || elem_stride <= 0 ||
      col_stride < 0)
    return (int)hipErrorInvalidValue;
  const int per_block = 256 * calib::kOrderPer;
  SGMCMC_LAUNCH(calib::order_kernel, dim3((unsigned)((n + per_block - 1) / per_block), (unsigned)ncols), dim3(256), 0,
                (hipStream_t)stream, keys, elem_stride, col_stride, n, perm);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_calibration_error(const double* keys, int64_t elem_stride, int64_t col_stride,
                                        const int32_t* perm, const int64_t* target, int class_conditional, int n,
                                        int ncols, const double* bounds, int num_bins, int l2, double* col_err,
                                        double* out, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!keys || !perm || !target || !col_err || !out || n <= 0 || n > calib::kMaxRows || ncols <= 0 ||
      ncols > 65535 || (!class_conditional && ncols != 1) || elem_stride <= 0 || col_stride < 0 || num_bins < 0 ||
      num_bins > calib::kMaxBins || (bounds && num_bins == 0))
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(calib::calib_kernel, dim3((unsigned)ncols), dim3(256), 0, (hipStream_t)stream, keys, elem_stride,
                col_stride, perm, target, class_conditional, n, bounds, num_bins, l2, col_err);
  SGMCMC_LAUNCH(calib::calib_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, col_err, ncols,
                class_conditional, l2, out);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_rank_metrics(const double* scores, const int32_t* perm, int n, int n_pos, double* out,
                                   void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!scores || !perm || !out || n <= 0 || n > calib::kMaxRows || n_pos <= 0 || n_pos >= n)
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(calib::rank_kernel, dim3(1), dim3(calib::kRankThreads), 0, (hipStream_t)stream, scores, perm, n,
                n_pos, out);
  return (int)hipGetLastError();
}
