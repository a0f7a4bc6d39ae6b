// Kernel Stein discrepancy and Stein thinning (include/sgmcmc_hip.h, "Kernel Stein discrepancy"): the Gram matrix of the
// 2S rows [X - x_0; G] on the fp64 matrix pipe, the Stein matrix K of the inverse multiquadric kernel, its row sums and
// quadratic forms, and the greedy thinning walk.  Included from sgmcmc_hip.hip after numerics_hip.inc (it uses num::qnan)
// and gram_hip.inc, which has the pieces the Gram pass shares with corr_hip.inc, its LDS layout and the MFMA lane map.
//
// What this Gram pass brings to the walk: the rows are samples and the contraction runs over the coordinates (unit stride:
// consecutive lanes always walk coordinates); row r of the 2S is sample r of X less the anchor x_0 (r < S) or score r - S
// (r >= S), decided row by row, since the X / G boundary falls inside a tile whenever S is no multiple of kTile.

namespace stein {

using gram::kThreads, gram::kTile, gram::kChunk, gram::kRow, gram::kPerThread, gram::tiles_of, gram::chunks_of;
constexpr int kMaxS = SGMCMC_STEIN_MAX_S;
constexpr int kMaxSplits = SGMCMC_STEIN_MAX_SPLITS;
constexpr int kTargetBlocks = SGMCMC_STEIN_TARGET_BLOCKS;
constexpr int kMaxBatch = SGMCMC_STEIN_MAX_BATCH;
constexpr int kStats = SGMCMC_STEIN_STATS;
constexpr int kMaxPicks = SGMCMC_STEIN_MAX_PICKS;
constexpr int kRowStep = kThreads / kChunk;            // a thread's elements of a tile: rows t / kChunk + kRowStep i
constexpr int kOwn = kMaxS / kThreads;                  // candidates a thread of the thinning walk owns
constexpr int64_t kMaxD = ((int64_t)1 << 31) - 1;
static_assert(kOwn * kThreads == kMaxS, "thinning geometry");

inline bool shape_ok(int S, int64_t D) { return S >= 2 && S <= kMaxS && D >= 1 && D <= kMaxD; }
inline int splits(int S, int64_t D, int64_t ws) { return gram::splits(2 * S, D, ws, kMaxSplits, kTargetBlocks); }

// row r of the 2S at coordinate col (< D): the element, as stored
template <typename T>
__device__ __forceinline__ T row_at(const T* __restrict__ x, const T* __restrict__ g, int S, int64_t xs, int64_t gs, int r,
                                    int64_t col) {
  return r < S ? x[(int64_t)r * xs + col] : g[(int64_t)(r - S) * gs + col];
}

// the tile of rows [rb, rb + kTile) at the coordinates [c kChunk, ..) -> registers (0 outside the matrix)
template <typename T>
__device__ __forceinline__ void load_tile(const T* __restrict__ x, const T* __restrict__ g, int S, int64_t D, int64_t xs,
                                          int64_t gs, int rb, int64_t c, T (&r)[kPerThread]) {
  const int64_t col = c * kChunk + (threadIdx.x % kChunk);
  const int r0 = rb + threadIdx.x / kChunk;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int row = r0 + kRowStep * i;
    r[i] = (row < 2 * S && col < D) ? row_at(x, g, S, xs, gs, row, col) : (T)0;
  }
}

// registers -> tile[row][coordinate] in fp64, the anchor a0 = x_0[col] subtracted from the rows of X; returns the
// thread's non-finite elements
template <typename T>
__device__ __forceinline__ int store_tile(double* tile, int S, int64_t D, int rb, int64_t c, T a0, const T (&r)[kPerThread]) {
  const int kk = threadIdx.x % kChunk, v0 = threadIdx.x / kChunk;
  const bool cin = c * kChunk + kk < D;
  int bad = 0;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int vv = v0 + kRowStep * i, row = rb + vv;
    const bool in = cin && row < 2 * S;
    const double xv = (double)r[i];
    bad += in && !(fabs(xv) <= 1.79769313486231570815e308);
    tile[vv * kRow + kk] = !in ? 0.0 : row < S ? xv - (double)a0 : xv;
  }
  return bad;
}

// ---- 1. Gram pass: slab[split] block (bi, bj), bi <= bj, = sum over the chunks split, split + splits, ... of r r^T ----
template <typename T>
__global__ __launch_bounds__(kThreads) void gram_kernel(const T* __restrict__ x, const T* __restrict__ g, int S, int64_t D,
                                                        int64_t xs, int64_t gs, int64_t nchunks, double* __restrict__ slabs,
                                                        long long* __restrict__ counts) {
  __shared__ double sA[kTile * kRow];
  __shared__ double sB[kTile * kRow];
  __shared__ int sBad;
  const int t = threadIdx.x, V = 2 * S;
  const int nb = (V + kTile - 1) / kTile;
  int p = blockIdx.x, bi = 0;
  while (p >= nb - bi) {                                // block pair p of the upper triangle, row-major
    p -= nb - bi;
    ++bi;
  }
  const int bj = bi + p, va = bi * kTile, vb = bj * kTile;
  const bool diag = bi == bj;
  const int split = blockIdx.y, nsplit = gridDim.y;
  if (t == 0) sBad = 0;
  int64_t c = split;                                    // (splits <= nchunks: every workgroup has a chunk)
  T ra[kPerThread], rb[kPerThread], a0;
  {
    const int64_t col = c * kChunk + (t % kChunk);
    a0 = col < D ? x[col] : (T)0;
  }
  load_tile(x, g, S, D, xs, gs, va, c, ra);
  if (!diag) load_tile(x, g, S, D, xs, gs, vb, c, rb);
  gram::f64x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = gram::f64x4{0.0, 0.0, 0.0, 0.0};
  const int lane = t & 63, wave = t >> 6;
  const double* tb = diag ? sA : sB;
  const double* pa = sA + ((wave >> 1) * 32 + (lane & 15)) * kRow + (lane >> 4);
  const double* pb = tb + ((wave & 1) * 32 + (lane & 15)) * kRow + (lane >> 4);
  int bad = 0;
  for (; c < nchunks; c += nsplit) {
    __syncthreads();                                    // the tiles of the chunk before are done with
    const int nbad = store_tile(sA, S, D, va, c, a0, ra);
    if (diag) bad += nbad;                              // (every row tile is on the diagonal once per split)
    else store_tile(sB, S, D, vb, c, a0, rb);
    __syncthreads();
    const int64_t next = c + nsplit;
    if (next < nchunks) {                               // the next chunk's loads fly while this one is multiplied
      const int64_t col = next * kChunk + (t % kChunk);
      a0 = col < D ? x[col] : (T)0;
      load_tile(x, g, S, D, xs, gs, va, next, ra);
      if (!diag) load_tile(x, g, S, D, xs, gs, vb, next, rb);
    }
#pragma unroll
    for (int k = 0; k < kChunk; k += 4) {
      const double a_0 = pa[k], a_1 = pa[16 * kRow + k], b_0 = pb[k], b_1 = pb[16 * kRow + k];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_0, b_0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_0, b_1, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_1, b_0, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_1, b_1, acc[3], 0, 0, 0);
    }
  }
  double* slab = slabs + (size_t)split * V * V;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int col = vb + (wave & 1) * 32 + (q & 1) * 16 + (lane & 15);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = va + (wave >> 1) * 32 + (q >> 1) * 16 + (lane >> 4) + 4 * reg;
      if (row < V && col < V) slab[(size_t)row * V + col] = acc[q][reg];
    }
  }
  if (diag) {
    if (bad) atomicAdd(&sBad, bad);                     // (an integer in LDS: exact in any order)
    __syncthreads();
    if (t == 0) counts[(size_t)split * nb + bi] = sBad;
  }
}

// ---- 2. reduce: gram[2S][2S] = the splits added in ascending order, mirrored; nonfinite[0] = the sum of the counts ------
__global__ __launch_bounds__(kThreads) void reduce_kernel(const double* __restrict__ slabs,
                                                          const long long* __restrict__ counts, int splits, int ncounts,
                                                          int V, double* __restrict__ gram, long long* __restrict__ nonfinite) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx == 0) {
    long long bad = 0;
    for (int b = 0; b < ncounts; ++b) bad += counts[b];
    nonfinite[0] = bad;
  }
  if (idx >= V * V) return;
  const int i = idx / V, j = idx - i * V, a = i < j ? i : j, b = i < j ? j : i;
  const size_t at[1] = {(size_t)a * V + b};
  double s[1];
  gram::slab_sums(slabs, splits, (size_t)V * V, at, s);
  gram[idx] = s[0];
}

// ---- 3. finish: r2 and the Stein matrix K of gram = [[A, B], [B^T, C]], entry (i, j) evaluated as (min, max) ---------------
__global__ __launch_bounds__(kThreads) void finish_kernel(const double* __restrict__ gram, int S, double d, double c2,
                                                          const double* __restrict__ c2_dev, double beta,
                                                          const long long* __restrict__ nonfinite, double* __restrict__ K,
                                                          double* __restrict__ r2_out) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= S * S) return;
  const int V = 2 * S, i0 = idx / S, j0 = idx - i0 * S, i = i0 < j0 ? i0 : j0, j = i0 < j0 ? j0 : i0;
  const bool bad = nonfinite[0] != 0;
  const double* gi = gram + (size_t)i * V;
  const double* gj = gram + (size_t)j * V;
  const double r2v = (gi[i] + gj[j]) - 2.0 * gi[j];
  const double r2 = r2v > 0.0 ? r2v : 0.0;
  if (r2_out) r2_out[idx] = bad ? num::qnan() : r2;
  if (!K) return;
  if (c2_dev) c2 = c2_dev[0];
  const double tt = ((gi[S + i] - gi[S + j]) - gj[S + i]) + gj[S + j];
  const double cij = gram[(size_t)(S + i) * V + S + j];
  const double u = c2 + r2;
  const double p0 = beta == -0.5 ? 1.0 / sqrt(u) : pow(u, beta), p1 = p0 / u, p2 = p1 / u;
  const double k = (p0 * cij - (2.0 * beta) * p1 * (tt + d)) - (4.0 * beta * (beta - 1.0)) * p2 * r2;
  K[idx] = bad ? num::qnan() : k;
}

// ---- 4. rows: rowsum[r][i] = sum_j W_rj K_ij (a wave per row: lane l adds j = l, l + 64, ... ascending, then the fixed
//         tree l += l + 32, ..., l + 1); row_mean = rowsum / S --------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void rows_kernel(const double* __restrict__ K, int S, const double* __restrict__ W,
                                                        double* __restrict__ rowsum, double* __restrict__ row_mean) {
  __shared__ double sh[kThreads];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = blockIdx.y;
  const int i = blockIdx.x * (kThreads / 64) + wave;
  const double* w = W ? W + (size_t)r * S : nullptr;
  double acc = 0.0;
  if (i < S)
    for (int j = lane; j < S; j += 64) acc += (w ? w[j] : 1.0) * K[(size_t)i * S + j];
  sh[t] = acc;
  __syncthreads();
  for (int off = 32; off > 0; off >>= 1) {
    if (lane < off) sh[t] += sh[t + off];
    __syncthreads();
  }
  if (lane == 0 && i < S) {
    rowsum[(size_t)r * S + i] = sh[t];
    if (row_mean) row_mean[(size_t)r * S + i] = sh[t] / (double)S;
  }
}

// ---- 5. forms: stats[r] = {Q = sum_i W_ri rowsum_ri / S^2, (sum - sum_i W_ri^2 K_ii) / (S (S - 1)), sqrt(Q)}: thread t
//         adds i = t, t + 256, ... ascending, then the fixed tree t += t + 128, ..., t + 1 -------------------------------------
__global__ __launch_bounds__(kThreads) void forms_kernel(const double* __restrict__ K, int S, const double* __restrict__ W,
                                                         const double* __restrict__ rowsum, double* __restrict__ stats) {
  __shared__ double sT[kThreads], sD[kThreads];
  const int t = threadIdx.x, r = blockIdx.x;
  const double* w = W ? W + (size_t)r * S : nullptr;
  double tot = 0.0, dia = 0.0;
  for (int i = t; i < S; i += kThreads) {
    const double wi = w ? w[i] : 1.0;
    tot += wi * rowsum[(size_t)r * S + i];
    dia += (wi * wi) * K[(size_t)i * S + i];
  }
  sT[t] = tot, sD[t] = dia;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (t < off) sT[t] += sT[t + off], sD[t] += sD[t + off];
    __syncthreads();
  }
  if (t == 0) {
    const double n = (double)S, v = sT[0] / (n * n);
    double* out = stats + (size_t)r * kStats;
    out[0] = v;
    out[1] = (sT[0] - sD[0]) / (n * (n - 1.0));
    out[2] = v < 0.0 ? 0.0 : sqrt(v);                   // (NaN stays NaN)
  }
}

// ---- 6. thinning: one workgroup, m trips; thread t owns the candidates t, t + 256, ... -----------------------------------
__device__ __forceinline__ bool before(double v, int i, double v2, int i2) { return v < v2 || (v == v2 && i < i2); }
__device__ __forceinline__ double objective(double half, double run) {     // (a NaN never wins: +inf, the last of all)
  const double v = half + run;
  return v == v ? v : INFINITY;
}

__global__ __launch_bounds__(kThreads) void thin_kernel(const double* __restrict__ K, int S, int m,
                                                        long long* __restrict__ indices, double* __restrict__ path) {
  __shared__ double sRun[kMaxS], sHalf[kMaxS], sV[kThreads];
  __shared__ int sI[kThreads];
  const int t = threadIdx.x;
  for (int j = t; j < S; j += kThreads) sRun[j] = 0.0, sHalf[j] = 0.5 * K[(size_t)j * S + j];
  double total = 0.0;                                   // (thread 0's: sum_{a, b <= trip} K(pi_a, pi_b))
  __syncthreads();
  for (int a = 0; a < m; ++a) {
    double bv = INFINITY;
    int bi = t < S ? t : S;                             // (S: no candidate; thread 0 always has one, so S never wins)
    if (t < S) bv = objective(sHalf[t], sRun[t]);
#pragma unroll
    for (int q = 1; q < kOwn; ++q) {
      const int j = t + q * kThreads;
      if (j < S) {
        const double v = objective(sHalf[j], sRun[j]);
        if (before(v, j, bv, bi)) bv = v, bi = j;
      }
    }
    sV[t] = bv, sI[t] = bi;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {  // the fixed tree; (value, index) is a total order: ties -> smaller j
      if (t < off && before(sV[t + off], sI[t + off], sV[t], sI[t])) sV[t] = sV[t + off], sI[t] = sI[t + off];
      __syncthreads();
    }
    const int pick = sI[0];                             // (< S: thread 0 has a candidate and S is the last of all)
    if (t == 0) {
      total += 2.0 * sRun[pick] + 2.0 * sHalf[pick];
      indices[a] = pick;
      path[a] = sqrt(total) / (double)(a + 1);
    }
    __syncthreads();                                    // sRun[pick] and sI[0] are read before anyone moves on
    const double* row = K + (size_t)pick * S;
#pragma unroll
    for (int q = 0; q < kOwn; ++q) {
      const int j = t + q * kThreads;
      if (j < S) sRun[j] += row[j];
    }
  }
}

}  // namespace stein

extern "C" int sgmcmc_stein_splits(int S, int64_t D, int64_t workspace_bytes) {
  if (!stein::shape_ok(S, D) || workspace_bytes < 0) return -1;
  return stein::splits(S, D, workspace_bytes);
}

extern "C" int sgmcmc_stein_gram(const void* x, const void* score, int dtype, int S, int64_t D, int64_t x_stride,
                                 int64_t score_stride, int splits, double* slabs, int64_t* counts, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !score || !slabs || !counts || !stein::shape_ok(S, D) || x_stride < 0 || score_stride < 0 || splits < 1 ||
      splits > stein::kMaxSplits || splits > stein::chunks_of(D) || (dtype != SGMCMC_F32 && dtype != SGMCMC_F64))
    return (int)hipErrorInvalidValue;
  const dim3 grid = gram::pair_grid(2 * S, splits), block(stein::kThreads);
  if (dtype == SGMCMC_F32)
    SGMCMC_LAUNCH(stein::gram_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, (const float*)score, S, D,
                  x_stride, score_stride, stein::chunks_of(D), slabs, (long long*)counts);
  else
    SGMCMC_LAUNCH(stein::gram_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x, (const double*)score, S,
                  D, x_stride, score_stride, stein::chunks_of(D), slabs, (long long*)counts);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_stein_reduce(const double* slabs, const int64_t* counts, int splits, int S, double* gram,
                                   int64_t* nonfinite, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!slabs || !counts || !gram || !nonfinite || S < 2 || S > stein::kMaxS || splits < 1 || splits > stein::kMaxSplits)
    return (int)hipErrorInvalidValue;
  const int V = 2 * S;
  SGMCMC_LAUNCH(stein::reduce_kernel, dim3((V * V + stein::kThreads - 1) / stein::kThreads), dim3(stein::kThreads), 0,
                (hipStream_t)stream, slabs, (const long long*)counts, splits, splits * stein::tiles_of(V), V, gram,
                (long long*)nonfinite);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_stein_finish(const double* gram, int S, double d, double c2, const double* c2_device, double beta,
                                   const int64_t* nonfinite, double* K, double* r2, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!gram || !nonfinite || (!K && !r2) || S < 2 || S > stein::kMaxS || !(d >= 1.0) || !(beta > -1.0 && beta < 0.0) ||
      (K && !c2_device && !(c2 > 0.0 && c2 < INFINITY)))
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(stein::finish_kernel, dim3((S * S + stein::kThreads - 1) / stein::kThreads), dim3(stein::kThreads), 0,
                (hipStream_t)stream, gram, S, d, c2, c2_device, beta, (const long long*)nonfinite, K, r2);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_stein_forms(const double* K, int S, const double* W, int R, double* rowsum, double* row_mean,
                                  double* stats, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!K || !rowsum || !stats || S < 2 || S > stein::kMaxS || R < 1 || R > stein::kMaxBatch || (!W && R != 1))
    return (int)hipErrorInvalidValue;
  const int per = stein::kThreads / 64;
  SGMCMC_LAUNCH(stein::rows_kernel, dim3((S + per - 1) / per, R), dim3(stein::kThreads), 0, (hipStream_t)stream, K, S, W,
                rowsum, row_mean);
  SGMCMC_LAUNCH(stein::forms_kernel, dim3(R), dim3(stein::kThreads), 0, (hipStream_t)stream, K, S, W,
                (const double*)rowsum, stats);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_stein_thin(const double* K, int S, int m, int64_t* indices, double* path, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!K || !indices || !path || S < 2 || S > stein::kMaxS || m < 1 || m > stein::kMaxPicks)
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(stein::thin_kernel, dim3(1), dim3(stein::kThreads), 0, (hipStream_t)stream, K, S, m, (long long*)indices,
                path);
  return (int)hipGetLastError();
}
