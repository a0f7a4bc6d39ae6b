// Weight-correlation analysis (include/sgmcmc_hip.h, "Correlation between the variables of a stack"): per-variable means,
// the centred Gram matrix G = d d^T on the fp64 matrix pipe, cov / corr and the off-diagonal statistics of a correlation
// matrix.  Included from sgmcmc_hip.hip after numerics_hip.inc (it uses num::comp_add and num::qnan) and gram_hip.inc,
// which has the pieces the Gram pass shares with stein_hip.inc, its LDS layout and the MFMA lane map.
//
// One loader serves the mean and the Gram pass: a tile of kTile variables x kChunk observations is read through the
// strided geometry with consecutive lanes on consecutive addresses -- along the variables when the variable stride is the
// smaller one (v_major), else along the observations -- and staged in LDS as tile[variable][observation] in fp64.  All
// arithmetic then reads the LDS tile, so the summation order is a function of (V, n) alone, whatever the strides are.

namespace corr {

using gram::kThreads, gram::kTile, gram::kChunk, gram::kRow, gram::kPerThread, gram::tiles_of, gram::chunks_of;
constexpr int kMaxV = SGMCMC_CORR_MAX_V;
constexpr int kMaxSplits = SGMCMC_CORR_MAX_SPLITS;
constexpr int kTargetBlocks = SGMCMC_CORR_TARGET_BLOCKS;
constexpr int kMeanBlocks = SGMCMC_CORR_MEAN_BLOCKS;
constexpr int kMaxBatch = SGMCMC_CORR_MAX_BATCH;
constexpr int kStats = SGMCMC_CORR_STATS;
constexpr int64_t kMaxN = ((int64_t)1 << 31) - 1;
typedef sgmcmc_corr_geometry Geom;

inline int splits(int V, int64_t n, int64_t ws) { return gram::splits(V, n, ws, kMaxSplits, kTargetBlocks); }
inline int mean_blocks(int V, int64_t n) {
  const int64_t chunks = chunks_of(n), cap = kMeanBlocks / tiles_of(V);
  return (int)(chunks < cap ? chunks : cap);
}
inline bool geometry_ok(const Geom* g) {
  if (!g || g->V < 1 || g->V > kMaxV || g->n < 2 || g->n > kMaxN || g->v_stride < 0) return false;
  int64_t prod = 1;
  for (int k = 0; k < 4; ++k) {
    if (g->size[k] < 1 || g->size[k] > kMaxN || g->stride[k] < 0 || prod > kMaxN) return false;
    prod *= g->size[k];
  }
  return prod == g->n;
}

// element offset of observation k (< 2^31 + kChunk): its index is decomposed over the observation dimensions
__device__ __forceinline__ int64_t obs_offset(const Geom& g, uint32_t k) {
  int64_t off = 0;
#pragma unroll
  for (int a = 3; a >= 0; --a) {
    const uint32_t s = (uint32_t)g.size[a];
    if (s != 1) {                                       // (uniform: unused dimensions cost no division)
      const uint32_t q = k / s;
      off += (int64_t)(k - q * s) * g.stride[a];
      k = q;
    }
  }
  return off;
}

// (variable, observation) of a tile that element i of thread t is: lanes walk whichever the strides make contiguous
__device__ __forceinline__ void tile_index(const Geom& g, int t, int i, int& vv, int& kk) {
  if (g.v_major) {
    vv = t & (kTile - 1);
    kk = t / kTile + (kThreads / kTile) * i;
  } else {
    kk = t % kChunk;
    vv = t / kChunk + (kThreads / kChunk) * i;
  }
}

// the tile of variables [vb, vb + kTile) at the chunk whose observation offsets are off[0 .. kvalid) -> registers
template <typename T>
__device__ __forceinline__ void load_tile(const T* __restrict__ x, const Geom& g, int vb, const int64_t* off, int kvalid,
                                          T (&r)[kPerThread]) {
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    int vv, kk;
    tile_index(g, threadIdx.x, i, vv, kk);
    const int v = vb + vv;
    r[i] = (v < g.V && kk < kvalid) ? x[(int64_t)v * g.v_stride + off[kk]] : (T)0;
  }
}

// registers -> tile[vv][kk] = x - centre[vv] in fp64 (0 outside the matrix); returns the thread's non-finite elements
template <typename T>
__device__ __forceinline__ int store_tile(double* tile, const double* centre, const Geom& g, int vb, int kvalid,
                                          const T (&r)[kPerThread]) {
  int bad = 0;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    int vv, kk;
    tile_index(g, threadIdx.x, i, vv, kk);
    const bool in = vb + vv < g.V && kk < kvalid;
    const double xv = (double)r[i];
    bad += in && !(fabs(xv) <= 1.79769313486231570815e308);
    tile[vv * kRow + kk] = in ? xv - centre[vv] : 0.0;
  }
  return bad;
}

__device__ __forceinline__ int valid_of(const Geom& g, int64_t chunk) {
  const int64_t left = g.n - chunk * kChunk;
  return (int)(left < kChunk ? left : kChunk);
}

// ---- 1. mean pass: part[seg][v] = sum over the chunks seg, seg + segs, ... of (x_v - x_v(0)); counts[block] ----------
template <typename T>
__global__ __launch_bounds__(kThreads) void mean_kernel(const T* __restrict__ x, const Geom g, int64_t nchunks,
                                                        double* __restrict__ part, long long* __restrict__ counts) {
  __shared__ double sTile[kTile * kRow];
  __shared__ double sShift[kTile];
  __shared__ int64_t sOff[kChunk];
  __shared__ double sSum[kThreads];
  __shared__ int sBad;
  const int t = threadIdx.x, vb = blockIdx.x * kTile, seg = blockIdx.y, segs = gridDim.y;
  if (t == 0) sBad = 0;
  if (t < kTile) {
    const double s = vb + t < g.V ? (double)x[(int64_t)(vb + t) * g.v_stride] : 0.0;
    sShift[t] = fabs(s) <= 1.79769313486231570815e308 ? s : 0.0;
  }
  double acc = 0.0, comp = 0.0;
  int bad = 0;
  T r[kPerThread];
  for (int64_t c = seg; c < nchunks; c += segs) {
    __syncthreads();                                    // the tile and sOff of the chunk before are done with
    if (t < kChunk) sOff[t] = obs_offset(g, (uint32_t)(c * kChunk + t));
    __syncthreads();
    const int kvalid = valid_of(g, c);
    load_tile(x, g, vb, sOff, kvalid, r);
    bad += store_tile(sTile, sShift, g, vb, kvalid, r);
    __syncthreads();
    // thread (v = t / 4, q = t % 4) adds observations q, q + 4, ... of the chunk from 0 in ascending order
    const double* row = sTile + (t >> 2) * kRow + (t & 3);
    double ts = 0.0;
#pragma unroll
    for (int k = 0; k < kChunk; k += 4) ts += row[k];
    num::comp_add(acc, comp, ts);                       // ... and the chunks' sums in ascending order, compensated
  }
  sSum[t] = acc + comp;
  if (bad) atomicAdd(&sBad, bad);                       // (an integer in LDS: exact in any order)
  __syncthreads();
  if ((t & 3) == 0 && vb + (t >> 2) < g.V)
    part[(size_t)seg * g.V + vb + (t >> 2)] = ((sSum[t] + sSum[t + 1]) + sSum[t + 2]) + sSum[t + 3];
  if (t == 0) counts[blockIdx.y * gridDim.x + blockIdx.x] = sBad;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void mean_finish_kernel(const T* __restrict__ x, const Geom g, int segs, int nblk,
                                                               const double* __restrict__ part,
                                                               const long long* __restrict__ counts,
                                                               double* __restrict__ mean, long long* __restrict__ nonfinite) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  long long bad = 0;
  for (int b = 0; b < nblk; ++b) bad += counts[b];
  if (v == 0) nonfinite[0] = bad;
  if (v >= g.V) return;
  double s = 0.0, c = 0.0;
  for (int q = 0; q < segs; ++q) num::comp_add(s, c, part[(size_t)q * g.V + v]);
  mean[v] = bad ? num::qnan() : (double)x[(int64_t)v * g.v_stride] + (s + c) / (double)g.n;
}

// ---- 2. Gram pass: slab[split][r] block (bi, bj), bi <= bj, = sum over the chunks split, split + splits, ... of d d^T --
template <typename T>
__global__ __launch_bounds__(kThreads) void gram_kernel(const T* __restrict__ x, const Geom g, int64_t batch_stride,
                                                        const double* __restrict__ mean, int64_t nchunks,
                                                        double* __restrict__ slabs) {
  __shared__ double sA[kTile * kRow];
  __shared__ double sB[kTile * kRow];
  __shared__ double sMean[2 * kTile];
  __shared__ int64_t sOff[2][kChunk];
  const int t = threadIdx.x;
  const int nb = (g.V + kTile - 1) / kTile;
  int p = blockIdx.x, bi = 0;
  while (p >= nb - bi) {                                // block pair p of the upper triangle, row-major
    p -= nb - bi;
    ++bi;
  }
  const int bj = bi + p, va = bi * kTile, vb = bj * kTile;
  const bool diag = bi == bj;
  const int split = blockIdx.y, splits = gridDim.y, rep = blockIdx.z, R = gridDim.z;
  x += (int64_t)rep * batch_stride;
  if (t < 2 * kTile) {
    const int v = t < kTile ? va + t : vb + t - kTile;
    sMean[t] = v < g.V ? mean[v] : 0.0;
  }
  int64_t c = split;                                    // (splits <= nchunks: every workgroup has a chunk)
  if (t < kChunk) sOff[0][t] = obs_offset(g, (uint32_t)(c * kChunk + t));
  __syncthreads();
  T ra[kPerThread], rb[kPerThread];
  load_tile(x, g, va, sOff[0], valid_of(g, c), ra);
  if (!diag) load_tile(x, g, vb, sOff[0], valid_of(g, c), rb);
  gram::f64x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = gram::f64x4{0.0, 0.0, 0.0, 0.0};
  const int lane = t & 63, wave = t >> 6;
  const double* tb = diag ? sA : sB;
  const double* pa = sA + ((wave >> 1) * 32 + (lane & 15)) * kRow + (lane >> 4);
  const double* pb = tb + ((wave & 1) * 32 + (lane & 15)) * kRow + (lane >> 4);
  for (int it = 0; c < nchunks; c += splits, ++it) {
    __syncthreads();                                    // the tiles of the chunk before are done with
    const int kvalid = valid_of(g, c);
    store_tile(sA, sMean, g, va, kvalid, ra);
    if (!diag) store_tile(sB, sMean + kTile, g, vb, kvalid, rb);
    const int64_t next = c + splits;
    int64_t* off = sOff[(it + 1) & 1];
    if (next < nchunks && t < kChunk) off[t] = obs_offset(g, (uint32_t)(next * kChunk + t));
    __syncthreads();
    if (next < nchunks) {                               // the next chunk's loads fly while this one is multiplied
      load_tile(x, g, va, off, valid_of(g, next), ra);
      if (!diag) load_tile(x, g, vb, off, valid_of(g, next), rb);
    }
#pragma unroll
    for (int k = 0; k < kChunk; k += 4) {
      const double a0 = pa[k], a1 = pa[16 * kRow + k], b0 = pb[k], b1 = pb[16 * kRow + k];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[3], 0, 0, 0);
    }
  }
  double* slab = slabs + ((size_t)split * R + rep) * g.V * g.V;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int col = vb + (wave & 1) * 32 + (q & 1) * 16 + (lane & 15);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = va + (wave >> 1) * 32 + (q >> 1) * 16 + (lane >> 4) + 4 * reg;
      if (row < g.V && col < g.V) slab[(size_t)row * g.V + col] = acc[q][reg];
    }
  }
}

// ---- 3. finish: G = the splits added in ascending order, mirrored; cov, corr, zero_variance ------------------------------
__global__ __launch_bounds__(kThreads) void finish_kernel(const double* __restrict__ slabs, int splits, int V, double denom,
                                                          const long long* __restrict__ nonfinite,
                                                          double* __restrict__ cov, double* __restrict__ corr,
                                                          unsigned char* __restrict__ zero_variance) {
  const int idx = blockIdx.x * kThreads + threadIdx.x, rep = blockIdx.y, R = gridDim.y;
  if (idx >= V * V) return;
  const int i = idx / V, j = idx - i * V, a = i < j ? i : j, b = i < j ? j : i;
  const size_t at[3] = {(size_t)a * V + b, (size_t)a * V + a, (size_t)b * V + b};
  double gs[3];
  gram::slab_sums(slabs + (size_t)rep * V * V, splits, (size_t)R * V * V, at, gs);
  const double gab = gs[0], gaa = gs[1], gbb = gs[2];
  const bool bad = nonfinite && nonfinite[0] != 0, flat = gaa == 0.0 || gbb == 0.0;
  const size_t o = (size_t)rep * V * V + idx;
  if (cov) cov[o] = bad ? num::qnan() : flat ? 0.0 : gab / denom;
  corr[o] = bad || flat ? num::qnan() : gab / sqrt(gaa * gbb);
  if (i == j) zero_variance[(size_t)rep * V + i] = !bad && gaa == 0.0;
}

// ---- 4. off-diagonal statistics of a correlation matrix, one workgroup per matrix ------------------------------------------
__device__ __forceinline__ bool better(double m, int i, int j, double m2, int i2, int j2) {   // (m, i, j) beats (m2, ..)?
  return i2 < 0 || (i >= 0 && (m > m2 || (m == m2 && (i < i2 || (i == i2 && j < j2)))));
}

__global__ __launch_bounds__(kThreads) void offdiag_kernel(const double* __restrict__ corr, int V, double* __restrict__ stats,
                                                           long long* __restrict__ counts) {
  __shared__ unsigned char sIn[kMaxV];
  __shared__ double sS[3][kThreads], sM[kThreads];
  __shared__ long long sN[kThreads];
  __shared__ int sI[kThreads], sJ[kThreads];
  const int t = threadIdx.x;
  corr += (size_t)blockIdx.x * V * V;
  for (int v = t; v < V; v += kThreads) {
    const double dv = corr[(size_t)v * V + v];
    sIn[v] = dv == dv;                                  // a variable without variance has a NaN diagonal
  }
  __syncthreads();
  double s[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0}, m = 0.0;
  long long cnt = 0;
  int mi = -1, mj = -1;
  for (int i = 0; i + 1 < V; ++i) {
    if (!sIn[i]) continue;
    for (int j = i + 1 + t; j < V; j += kThreads) {
      if (!sIn[j]) continue;
      const double r = corr[(size_t)i * V + j], ar = fabs(r);
      num::comp_add(s[0], c[0], r);
      num::comp_add(s[1], c[1], ar);
      num::comp_add(s[2], c[2], r * r);
      ++cnt;
      if (mi < 0 || ar > m) m = ar, mi = i, mj = j;     // (rows and columns ascend: the first of a tie stays)
    }
  }
  for (int q = 0; q < 3; ++q) sS[q][t] = s[q] + c[q];
  sM[t] = m, sN[t] = cnt, sI[t] = mi, sJ[t] = mj;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (t < off) {
      for (int q = 0; q < 3; ++q) sS[q][t] += sS[q][t + off];
      sN[t] += sN[t + off];
      if (better(sM[t + off], sI[t + off], sJ[t + off], sM[t], sI[t], sJ[t]))
        sM[t] = sM[t + off], sI[t] = sI[t + off], sJ[t] = sJ[t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double np = (double)sN[0];
    double* out = stats + (size_t)blockIdx.x * kStats;
    long long* cn = counts + (size_t)blockIdx.x * 3;
    const bool none = sN[0] == 0;
    out[0] = none ? num::qnan() : sS[0][0] / np;
    out[1] = none ? num::qnan() : sS[1][0] / np;
    out[2] = none ? num::qnan() : sqrt(sS[2][0] / np);
    out[3] = none ? num::qnan() : sM[0];
    out[4] = none ? num::qnan() : sS[2][0];
    cn[0] = sN[0], cn[1] = sI[0], cn[2] = sJ[0];
  }
}

}  // namespace corr

extern "C" int sgmcmc_corr_splits(int V, int64_t n, int64_t workspace_bytes) {
  if (V < 1 || V > corr::kMaxV || n < 2 || n > corr::kMaxN || workspace_bytes < 0) return -1;
  return corr::splits(V, n, workspace_bytes);
}

extern "C" int sgmcmc_corr_mean_blocks(int V, int64_t n) {
  if (V < 1 || V > corr::kMaxV || n < 2 || n > corr::kMaxN) return -1;
  return corr::mean_blocks(V, n);
}

extern "C" int sgmcmc_corr_mean(const void* w, int dtype, const sgmcmc_corr_geometry* geometry, double* part,
                                int64_t* counts, double* mean, int64_t* nonfinite, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!w || !corr::geometry_ok(geometry) || !part || !counts || !mean || !nonfinite ||
      (dtype != SGMCMC_F32 && dtype != SGMCMC_F64))
    return (int)hipErrorInvalidValue;
  const corr::Geom g = *geometry;
  const int segs = corr::mean_blocks(g.V, g.n), nb = corr::tiles_of(g.V);
  const int64_t nchunks = corr::chunks_of(g.n);
  const dim3 grid(nb, segs), block(corr::kThreads), fgrid((g.V + corr::kThreads - 1) / corr::kThreads);
  if (dtype == SGMCMC_F32) {
    SGMCMC_LAUNCH(corr::mean_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)w, g, nchunks, part,
                  (long long*)counts);
    SGMCMC_LAUNCH(corr::mean_finish_kernel<float>, fgrid, block, 0, (hipStream_t)stream, (const float*)w, g, segs,
                  nb * segs, (const double*)part, (const long long*)counts, mean, (long long*)nonfinite);
  } else {
    SGMCMC_LAUNCH(corr::mean_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)w, g, nchunks, part,
                  (long long*)counts);
    SGMCMC_LAUNCH(corr::mean_finish_kernel<double>, fgrid, block, 0, (hipStream_t)stream, (const double*)w, g, segs,
                  nb * segs, (const double*)part, (const long long*)counts, mean, (long long*)nonfinite);
  }
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_corr_gram(const void* x, int dtype, const sgmcmc_corr_geometry* geometry, int R,
                                int64_t batch_stride, const double* mean, int splits, double* slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !corr::geometry_ok(geometry) || !mean || !slabs || R < 1 || R > corr::kMaxBatch || batch_stride < 0 ||
      splits < 1 || splits > corr::kMaxSplits || splits > corr::chunks_of(geometry->n) ||
      (dtype != SGMCMC_F32 && dtype != SGMCMC_F64))
    return (int)hipErrorInvalidValue;
  const corr::Geom g = *geometry;
  const dim3 grid = gram::pair_grid(g.V, splits, R), block(corr::kThreads);
  if (dtype == SGMCMC_F32)
    SGMCMC_LAUNCH(corr::gram_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)x, g, batch_stride, mean,
                  corr::chunks_of(g.n), slabs);
  else
    SGMCMC_LAUNCH(corr::gram_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)x, g, batch_stride, mean,
                  corr::chunks_of(g.n), slabs);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_corr_finish(const double* slabs, int splits, int R, int V, int64_t n, int ddof,
                                  const int64_t* nonfinite, double* cov, double* corr_out, uint8_t* zero_variance,
                                  void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!slabs || !corr_out || !zero_variance || splits < 1 || splits > corr::kMaxSplits || R < 1 || R > corr::kMaxBatch ||
      V < 1 || V > corr::kMaxV || n < 2 || n > corr::kMaxN || ddof < 0 || ddof >= n)
    return (int)hipErrorInvalidValue;
  const dim3 grid((V * V + corr::kThreads - 1) / corr::kThreads, R), block(corr::kThreads);
  SGMCMC_LAUNCH(corr::finish_kernel, grid, block, 0, (hipStream_t)stream, slabs, splits, V, (double)(n - ddof),
                (const long long*)nonfinite, cov, corr_out, zero_variance);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_corr_offdiag(const double* corr_in, int R, int V, double* stats, int64_t* counts, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!corr_in || !stats || !counts || R < 1 || V < 1 || V > corr::kMaxV) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(corr::offdiag_kernel, dim3(R), dim3(corr::kThreads), 0, (hipStream_t)stream, corr_in, V, stats,
                (long long*)counts);
  return (int)hipGetLastError();
}
