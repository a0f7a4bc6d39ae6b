// Power-scaling sensitivity of stored draws (Kallioinen, Paananen, Buerkner, Vehtari 2023; the R package priorsense):
// how far every quantity's distribution moves when the prior, or the likelihood, is raised to a power near 1 by
// importance-reweighting the draws.  include/sgmcmc_hip.h states the definition.  The weights are model_comparison.psis'
// (psis_hip.inc as it is); this file has the two steps that it does not have.
//
// x[m][s][q], draw t = m S + s, N = M S draws, no splitting.
//
//   sort_kernel      the keyed column sort: a workgroup stages an [N_pad][TQ] tile of TQ columns in LDS as two arrays, the
//                    fp64 values and the uint16 draw indices (10 bytes per cell, kTileCells = 8,192 cells: 80 KiB), and
//                    sorts every column along N, ascending by value, ties by ascending draw index, with
//                    num::bitonic_walk -- the walk of summary::sort_kernel, which carries the keys here.  The order is
//                    total, so sorted[i][q] and order[i][q] are fixed whatever the network.  The non-finite rule is
//                    decided on load, before the padding rows are filled with (+inf, own row): such a column is written
//                    as (NaN, i).  Zeros are staged as +0.0.
//                    LDS layout: q is the fastest index of both arrays AND of the thread numbering, as in
//                    summary_hip.inc, whose argument holds for the values as it stands: the 32 lanes that ds_read_b64
//                    serves together read runs of j TQ consecutive doubles, conflict-free whenever j TQ >= 32, 2-way at
//                    worst in the last steps of a merge.  The keys are read by ds_read_u16 at the same cell numbers:
//                    32 lanes on runs of j TQ consecutive uint16, two lanes to a dword (one address: a broadcast) and the
//                    dwords of a 64-byte run on 16 distinct banks; a key store puts two lanes' halves into one dword of
//                    one bank, the same 2-way worst case.  No lane group strides along N.  Global loads and stores run
//                    along q.
//   distance_kernel  lane = quantity (summary::hdi_kernel's walk: row i of sorted and of order is one coalesced read of 8
//                    and of 2 bytes per lane), blockIdx.y = weight vector.  The weight vector w[.][a] is staged in LDS,
//                    8 N bytes (64 KiB at 8,192 draws).  W and the validity of the vector are formed by every thread from
//                    LDS over ascending t: all lanes read one address, a broadcast, no conflict.  The gather
//                    w[order[i][q]] is one ds_read_b64 per lane and row at an address that the data chooses: the 32 lanes
//                    of a group fall on the 32 bank pairs at random, about 3 to 4 distinct addresses on the fullest
//                    pair for unrelated columns (3 to 4 LDS cycles per group, 32 if every lane hits one pair with a
//                    different draw), and a broadcast where neighbouring quantities are ordered alike (the
//                    probabilities of one test row).  No padding or swizzle changes that for an index the data
//                    chooses.  It does not set the pace: a row costs a lane three fp64 divisions and g's sixteen Horner
//                    steps (or two log1p), some 150 fp64 instructions per wave and row against at most 8 LDS cycles for
//                    the gather.  Two walks over the column: C, den, num and sum w v; then sum w (v - wmean)^2.
//
// No atomics; every sum over ascending index with one accumulator; a quantity's result is a function of its own column
// and its weight vector only, whatever the grid, the tile or the chunk.

namespace powerscale {

constexpr int kMinDraws = SGMCMC_PSIS_MIN_DRAWS;              // what PSIS needs
constexpr int kMaxDraws = SGMCMC_POWERSCALE_MAX_DRAWS;        // N
constexpr int kTileCells = SGMCMC_POWERSCALE_TILE_CELLS;      // cells of the sort's tile: an fp64 value and a uint16 index
constexpr int kMaxTile = 64;                                  // TQ at most
constexpr int kSortThreads = 1024;
constexpr int kThreads = 256;
constexpr int kMaxVectors = 65535;                            // A: the grid's y
constexpr int kSeriesTerms = 16;
constexpr double kTwoLn2 = 1.3862943611198906;                // the double nearest 2 ln 2
static_assert((kMaxDraws & (kMaxDraws - 1)) == 0 && kTileCells >= kMaxDraws && kMaxDraws <= 65536, "one column fits");
static_assert((size_t)kTileCells * 10 + kMaxTile * sizeof(int) <= 160 * 1024, "LDS ceiling");
static_assert((size_t)kMaxDraws * sizeof(double) <= 160 * 1024, "LDS ceiling");

inline int padded(int N) {
  int p = 8;
  while (p < N) p <<= 1;
  return p;
}

inline int tile_quantities(int N) {
  if (N < kMinDraws || N > kMaxDraws) return 0;
  const int t = kTileCells / padded(N);
  return t < kMaxTile ? t : kMaxTile;
}

// N = chains * draws of a shape the sort takes, 0 otherwise
inline int total_draws(int64_t chain_stride, int64_t draw_stride, int chains, int draws, int64_t quantities) {
  if (chains <= 0 || draws <= 0 || quantities <= 0 || chain_stride < 0 || draw_stride < 0) return 0;
  const int64_t N = (int64_t)chains * draws;
  return N >= kMinDraws && N <= kMaxDraws ? (int)N : 0;
}

inline bool grid_of(int64_t quantities, int per_block, unsigned* blocks) {
  const int64_t b = (quantities + per_block - 1) / per_block;
  if (b > 0x7fffffffll) return false;
  *blocks = (unsigned)b;
  return true;
}

template <typename T>
__global__ __launch_bounds__(kSortThreads) void sort_kernel(const T* __restrict__ x, int64_t chain_stride,
                                                            int64_t draw_stride, int S, int64_t Q, int N, int n_pad,
                                                            int log_tq, double* __restrict__ sorted,
                                                            uint16_t* __restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) unsigned char powerscale_lds[];
  const int tq = 1 << log_tq, cells = n_pad << log_tq;
  double* __restrict__ tile = reinterpret_cast<double*>(powerscale_lds);          // [n_pad][tq]
  uint16_t* __restrict__ key = reinterpret_cast<uint16_t*>(tile + cells);         // [n_pad][tq]: the draw index
  int* __restrict__ bad = reinterpret_cast<int*>(key + cells);                    // [tq]: the column has a non-finite draw
  const int t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x << log_tq;

  if (t < tq) bad[t] = 0;
  __syncthreads();
  for (int e = t; e < cells; e += kSortThreads) {
    const int i = e >> log_tq, c = e & (tq - 1);
    double v = INFINITY;                          // padding: after every finite value, its index past every real one
    if (i < N) {
      v = 0.0;                                    // a column past the end of the call: sorted, never stored
      if (q0 + c < Q) {
        const int m = i / S, s = i - m * S;
        const double r = (double)x[(int64_t)m * chain_stride + (int64_t)s * draw_stride + q0 + c];
        v = r == 0.0 ? 0.0 : r;                   // -0.0 is staged as +0.0
        if (!num::is_finite(v)) bad[c] = 1;       // every writer stores the same value
      }
    }
    tile[e] = v;
    key[e] = (uint16_t)i;
  }

  num::bitonic_walk<true, kSortThreads>(tile, key, n_pad, log_tq);
  __syncthreads();

  for (int e = t; e < (N << log_tq); e += kSortThreads) {
    const int i = e >> log_tq, c = e & (tq - 1);
    if (q0 + c < Q) {
      sorted[(int64_t)i * Q + q0 + c] = bad[c] ? NAN : tile[e];
      order[(int64_t)i * Q + q0 + c] = bad[c] ? (uint16_t)i : key[e];         // unspecified, and inside [0, N)
    }
  }
}

// g(delta) = (1 - delta) log1p(-delta) + (1 + delta) log1p(delta), delta in [-1, 1]: the series in delta^2 below 1/4
__device__ __forceinline__ double g_of(double delta) {
  if (fabs(delta) < 0.25) {
    const double x = __dmul_rn(delta, delta);
    double acc = 0.0;
#pragma unroll
    for (int k = kSeriesTerms; k >= 1; --k) acc = __dmul_rn(__dadd_rn(acc, 1.0 / (double)(k * (2 * k - 1))), x);
    return acc;
  }
  const double t1 = delta >= 1.0 ? 0.0 : __dmul_rn(__dsub_rn(1.0, delta), log1p(-delta));     // 0 (-inf) = 0
  const double t2 = delta <= -1.0 ? 0.0 : __dmul_rn(__dadd_rn(1.0, delta), log1p(delta));
  return __dadd_rn(t1, t2);
}

__global__ __launch_bounds__(kThreads) void distance_kernel(const double* __restrict__ sorted,
                                                            const uint16_t* __restrict__ order, int N, int64_t Q,
                                                            const double* __restrict__ w, int A, int64_t out_stride,
                                                            double* __restrict__ dist_out, double* __restrict__ mean_out,
                                                            double* __restrict__ sd_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char powerscale_lds[];
  double* __restrict__ wl = reinterpret_cast<double*>(powerscale_lds);            // [N]: the weight vector
  const int a = blockIdx.y;
  for (int t = threadIdx.x; t < N; t += kThreads) wl[t] = w[(int64_t)t * A + a];
  __syncthreads();

  double W = 0.0;
  bool valid = true;
  for (int t = 0; t < N; ++t) {                   // one address for all lanes
    const double u = wl[t];
    valid = valid && u >= 0.0 && u < INFINITY;    // false for NaN as well
    W = __dadd_rn(W, u);
  }
  valid = valid && W > 0.0 && W < INFINITY;

  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= Q) return;                             // no barrier below
  const double* __restrict__ col = sorted + q;
  const uint16_t* __restrict__ ord = order + q;
  const int64_t out = (int64_t)a * out_stride + q;
  const double first = col[0];
  if (!valid || first != first) {                 // a column with a non-finite draw is NaN throughout
    dist_out[out] = NAN;
    mean_out[out] = NAN;
    sd_out[out] = NAN;
    return;
  }

  const double Nd = (double)N;
  double v = first, C = 0.0, top = 0.0, den = 0.0, swv = 0.0;
  for (int i = 0; i < N; ++i) {
    const int o = ord[(int64_t)i * Q];
    const double wi = wl[o < N ? o : 0];          // `order` as the sort wrote it is below N
    swv = __dadd_rn(swv, __dmul_rn(wi, v));
    if (i == N - 1) break;
    C = __dadd_rn(C, wi);
    const double next = col[(int64_t)(i + 1) * Q];
    const double Qi = __ddiv_rn(C, W), Pi = __ddiv_rn((double)(i + 1), Nd);
    const double s = __dadd_rn(Pi, Qi), delta = __ddiv_rn(__dsub_rn(Qi, Pi), s);
    const double ds = __dmul_rn(__dsub_rn(next, v), s);
    den = __dadd_rn(den, ds);
    top = __dadd_rn(top, __dmul_rn(ds, g_of(delta)));
    v = next;
  }
  const bool constant = first == v;               // sorted: every draw equals the first
  const double mean = constant ? first : __ddiv_rn(swv, W);

  double m2 = 0.0;
  for (int i = 0; i < N; ++i) {
    const int o = ord[(int64_t)i * Q];
    const double c = __dsub_rn(col[(int64_t)i * Q], mean);
    m2 = __dadd_rn(m2, __dmul_rn(wl[o < N ? o : 0], __dmul_rn(c, c)));
  }
  dist_out[out] = den == 0.0 ? 0.0 : sqrt(__ddiv_rn(__ddiv_rn(top, kTwoLn2), den));
  mean_out[out] = mean;
  sd_out[out] = constant ? 0.0 : sqrt(__ddiv_rn(m2, W));
}

// above 64 KiB of LDS per workgroup has to be asked for
inline hipError_t allow_lds(std::initializer_list<const void*> kernels, int most, bool* done) {
  if (*done) return hipSuccess;
  for (const void* k : kernels) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, most);
    if (e != hipSuccess) return e;
  }
  *done = true;
  return hipSuccess;
}

}  // namespace powerscale

extern "C" int sgmcmc_powerscale_tile_quantities(int total_draws) { return powerscale::tile_quantities(total_draws); }

extern "C" int sgmcmc_powerscale_sort(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains,
                                      int draws, int64_t quantities, double* sorted, uint16_t* order, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const int N = powerscale::total_draws(chain_stride, draw_stride, chains, draws, quantities);
  if (!x || !sorted || !order || N == 0) return (int)hipErrorInvalidValue;
  const int n_pad = powerscale::padded(N), tq = powerscale::tile_quantities(N);
  int log_tq = 0;
  while ((1 << log_tq) < tq) ++log_tq;
  unsigned blocks;
  if (!powerscale::grid_of(quantities, tq, &blocks)) return (int)hipErrorInvalidValue;
  static bool attr_done = false;
  const hipError_t e = powerscale::allow_lds({reinterpret_cast<const void*>(powerscale::sort_kernel<float>),
                                              reinterpret_cast<const void*>(powerscale::sort_kernel<double>)},
                                             powerscale::kTileCells * 10 + powerscale::kMaxTile * (int)sizeof(int),
                                             &attr_done);
  if (e != hipSuccess) return (int)e;
  const size_t lds = (size_t)n_pad * tq * 10 + (size_t)tq * sizeof(int);
  const dim3 grid(blocks), block(powerscale::kSortThreads);
  if (is_f64) SGMCMC_LAUNCH(powerscale::sort_kernel<double>, grid, block, lds, (hipStream_t)stream, (const double*)x,
                            chain_stride, draw_stride, draws, quantities, N, n_pad, log_tq, sorted, order);
  else SGMCMC_LAUNCH(powerscale::sort_kernel<float>, grid, block, lds, (hipStream_t)stream, (const float*)x,
                     chain_stride, draw_stride, draws, quantities, N, n_pad, log_tq, sorted, order);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_powerscale_distance(const double* sorted, const uint16_t* order, int total_draws,
                                          int64_t quantities, const double* weights, int vectors, int64_t out_stride,
                                          double* dist, double* wmean, double* wsd, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  unsigned blocks;
  if (!sorted || !order || !weights || !dist || !wmean || !wsd || total_draws < powerscale::kMinDraws ||
      total_draws > powerscale::kMaxDraws || quantities <= 0 || vectors <= 0 || vectors > powerscale::kMaxVectors ||
      out_stride < quantities || !powerscale::grid_of(quantities, powerscale::kThreads, &blocks))
    return (int)hipErrorInvalidValue;
  static bool attr_done = false;
  const hipError_t e = powerscale::allow_lds({reinterpret_cast<const void*>(powerscale::distance_kernel)},
                                             powerscale::kMaxDraws * (int)sizeof(double), &attr_done);
  if (e != hipSuccess) return (int)e;
  SGMCMC_LAUNCH(powerscale::distance_kernel, dim3(blocks, (unsigned)vectors), dim3(powerscale::kThreads),
                (size_t)total_draws * sizeof(double), (hipStream_t)stream, sorted, order, total_draws, quantities,
                weights, vectors, out_stride, dist, wmean, wsd);
  return (int)hipGetLastError();
}
