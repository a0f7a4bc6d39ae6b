// The Rao-Blackwellised regression model's marginal likelihood (fp64, deterministic; definitions in
// include/sgmcmc_hip.h, restated in tests/raob_reference.py).  With f [N, F] the features of the training rows, y [N],
// s2 the last layer's prior variance and v the noise variance:  G = f^T f, c = f^T y, yy = y^T y, A = s2 G + v I = L L^T.
//
//   gram_kernel     rows are cut into tiles of kRows; workgroup b of blocks(N) takes tiles b, b + blocks, ...  A tile is
//                   staged in LDS as fp64 with y as column F, so that G, c and yy are ONE lower triangle of order F + 1.
//                   A thread owns a 4 x 4 block of it (and, where F is small, one slice of the tile's rows): plain fp64
//                   FMAs from registers, the tiles' sums added compensated.  One partial record per workgroup.
//   factor_kernel   one workgroup of 1024: adds the partials in ascending order (compensated), then the right-looking Cholesky
//                   and the forward substitution for L^-1 in ONE sweep over the columns: at column j the whole workgroup
//                   scales column j of L and row j of L^-1, then applies the rank-1 update to what is left of A and of
//                   L^-1.  One padded square in LDS holds L below the diagonal and L^-T above it.  Every entry is
//                   updated in ascending j, i.e. in the order of the textbook's sequential loops.
//   grad_kernel     d log p / d f, row n: upstream (-s2 A^-1 f_n + (s2 / v) r_n b), r_n = y_n - s2 f_n . b
//   predict_kernel  mean s2 f* . b and variance v s2 |L^-1 f*|^2 + v per row of f*
//
// No atomics, no allocation, no host round trip; tile and grid are functions of (N, F) alone.

namespace raob {

constexpr int kMaxF = SGMCMC_RAOB_MAX_F;
constexpr int kThreads = 256;
constexpr int kRows = SGMCMC_RAOB_TILE_ROWS;             // rows of one Gram tile
constexpr int kMaxBlocks = SGMCMC_RAOB_MAX_BLOCKS;
constexpr int kScalars = SGMCMC_RAOB_SCALARS;
constexpr int kBlk = 4;                                  // a thread's block of the triangle is kBlk x kBlk
constexpr int kMaxOrder = kMaxF + 1;                     // y is column F
constexpr int kMaxB = (kMaxOrder + kBlk - 1) / kBlk;     // blocks along one side
constexpr int kStride = kMaxB * kBlk + 1;                // staged row: every block is readable, odd
constexpr int kSq = kMaxF + 1;                           // row stride of the factor's square
constexpr int kRowTile = 32, kLanes = kThreads / kRowTile;   // grad / predict: rows of a tile, threads of a row
constexpr int64_t kMaxN = 0x7fffffffll;
static_assert(kMaxB * (kMaxB + 1) / 2 <= kThreads, "a thread per block of the triangle");
static_assert(kRows * kStride >= kThreads * kBlk * kBlk, "the slices meet in the staging buffer");
static_assert(kStride % 2 == 1 && kSq % 2 == 1, "odd strides");
// the factor pass: one workgroup of kFactorThreads; thread (i, m) of kMaxF x kCols holds kPerRow entries of row i
constexpr int kFactorThreads = 1024, kCols = kFactorThreads / kMaxF, kPerRow = kMaxF / kCols;
constexpr int kOwn = 3, kBatch = 8;                      // partial-record entries a thread adds; records per batch
static_assert(kCols * kMaxF == kFactorThreads && kPerRow * kCols == kMaxF, "rows x columns");
static_assert(((kMaxOrder * (kMaxOrder + 1) / 2) + kFactorThreads - 1) / kFactorThreads <= kOwn, "entries a thread adds");

// scalars of the state record
enum { kLogLik = 0, kDv = 1, kV = 2, kS2 = 3, kLogDet = 4, kQuad = 5, kBB = 6, kTrace = 7, kYY = 8, kN = 9, kF = 10 };

__host__ __device__ inline int part_doubles(int F) { return (F + 1) * (F + 2) / 2; }
__host__ __device__ inline int off_b(int F) { (void)F; return kScalars; }
__host__ __device__ inline int off_linv(int F) { return kScalars + F; }
__host__ __device__ inline int off_ainv(int F) { return kScalars + F + F * F; }
__host__ __device__ inline int off_g(int F) { return kScalars + F + 2 * F * F; }
__host__ __device__ inline int off_c(int F) { return kScalars + F + 3 * F * F; }
__host__ __device__ inline int off_l(int F) { return kScalars + 2 * F + 3 * F * F; }
static_assert(SGMCMC_RAOB_STATE_DOUBLES(7) == kScalars + 2 * 7 + 4 * 49, "state record");

inline int blocks(int64_t N) {
  const int64_t tiles = (N + kRows - 1) / kRows;
  return (int)(tiles < kMaxBlocks ? tiles : kMaxBlocks);
}
inline int row_blocks(int64_t rows) {
  const int64_t tiles = (rows + kRowTile - 1) / kRowTile;
  return (int)(tiles < 4 * kMaxBlocks ? tiles : 4 * kMaxBlocks);
}
inline bool sizes_ok(int64_t N, int F) { return N >= 1 && N <= kMaxN && F >= 1 && F <= kMaxF; }

// entry e of a packed lower triangle -> (a, b), b <= a
__device__ __forceinline__ void unpack(int e, int& a, int& b) {
  a = 0;
  while ((a + 1) * (a + 2) / 2 <= e) ++a;
  b = e - a * (a + 1) / 2;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void gram_kernel(const T* __restrict__ f, const T* __restrict__ y, int64_t N, int F,
                                                        double* __restrict__ part) {
  __shared__ double sf[kRows * kStride];
  const int t = threadIdx.x;
  const int order = F + 1, B = (order + kBlk - 1) / kBlk, nb = B * (B + 1) / 2;
  const int S = kThreads / nb;                           // row slices of a block (>= 1)
  const int q = t / nb, e = t - q * nb;
  const bool active = q < S;
  int bi, bj;
  unpack(e, bi, bj);
  for (int i = t; i < kRows * kStride; i += kThreads) sf[i] = 0.0;   // the columns beyond F stay zero
  double acc[kBlk][kBlk], comp[kBlk][kBlk];
#pragma unroll
  for (int i = 0; i < kBlk; ++i)
#pragma unroll
    for (int j = 0; j < kBlk; ++j) acc[i][j] = comp[i][j] = 0.0;
  const int64_t tiles = (N + kRows - 1) / kRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRows;
    const int rows = (int)(N - row0 < kRows ? N - row0 : kRows), total = rows * F;
    const T* __restrict__ src = f + row0 * F;
    __syncthreads();                                     // the last tile has been read
    for (int k = t; k < total; k += kThreads) {
      const int r = k / F;
      sf[r * kStride + (k - r * F)] = (double)src[k];
    }
    if (t < rows) sf[t * kStride + F] = (double)y[row0 + t];
    __syncthreads();
    if (active) {
      double ta[kBlk][kBlk];
#pragma unroll
      for (int i = 0; i < kBlk; ++i)
#pragma unroll
        for (int j = 0; j < kBlk; ++j) ta[i][j] = 0.0;
      for (int r = q; r < rows; r += S) {
        const double* __restrict__ row = sf + r * kStride;
        double a[kBlk], b[kBlk];
#pragma unroll
        for (int i = 0; i < kBlk; ++i) {
          a[i] = row[bi * kBlk + i];
          b[i] = row[bj * kBlk + i];
        }
#pragma unroll
        for (int i = 0; i < kBlk; ++i)
#pragma unroll
          for (int j = 0; j < kBlk; ++j) ta[i][j] = fma(a[i], b[j], ta[i][j]);
      }
#pragma unroll
      for (int i = 0; i < kBlk; ++i)
#pragma unroll
        for (int j = 0; j < kBlk; ++j) num::comp_add(acc[i][j], comp[i][j], ta[i][j]);
    }
  }
  __syncthreads();
  // the slices of a block meet in the staging buffer, slice 0 adds them in ascending order
  if (active) {
#pragma unroll
    for (int i = 0; i < kBlk; ++i)
#pragma unroll
      for (int j = 0; j < kBlk; ++j) sf[(q * nb + e) * (kBlk * kBlk) + i * kBlk + j] = acc[i][j] + comp[i][j];
  }
  __syncthreads();
  if (active && q == 0) {
    double* __restrict__ out = part + (int64_t)blockIdx.x * part_doubles(F);
#pragma unroll
    for (int i = 0; i < kBlk; ++i)
#pragma unroll
      for (int j = 0; j < kBlk; ++j) {
        const int a = bi * kBlk + i, b = bj * kBlk + j;
        if (a < order && b <= a) {
          double s = sf[e * (kBlk * kBlk) + i * kBlk + j], c = 0.0;
          for (int p = 1; p < S; ++p) num::comp_add(s, c, sf[(p * nb + e) * (kBlk * kBlk) + i * kBlk + j]);
          out[a * (a + 1) / 2 + b] = s + c;
        }
      }
  }
}

__global__ __launch_bounds__(kFactorThreads) void factor_kernel(const double* __restrict__ part, int nblocks, int64_t N,
                                                                int F, double s2, double v_host,
                                                                const double* __restrict__ v_dev,
                                                                double* __restrict__ state) {
  __shared__ double sq[kMaxF * kSq];                     // L below the diagonal, L^-T above it
  __shared__ double sdg[kMaxF], sxd[kMaxF];              // the diagonals of L and of L^-1
  __shared__ double sc[kMaxF], sw[kMaxF], sb[kMaxF], srow[kMaxF], slog[kMaxF];
  __shared__ double ssum[4];
  const int t = threadIdx.x;
  const double v = v_dev ? *v_dev : v_host;
  const int E = part_doubles(F);
  {
    // a thread's entries, kBatch partial records at a time: the loads of a batch are in flight together, the sums stay
    // in ascending order of the workgroups (a record beyond the last adds 0, which changes nothing)
    double s[kOwn], c[kOwn];
    int at[kOwn];
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      s[i] = c[i] = 0.0;
      at[i] = t + i * kFactorThreads < E ? t + i * kFactorThreads : E - 1;
    }
    for (int p0 = 0; p0 < nblocks; p0 += kBatch) {
      double val[kBatch][kOwn];
#pragma unroll
      for (int q = 0; q < kBatch; ++q)
#pragma unroll
        for (int i = 0; i < kOwn; ++i) val[q][i] = p0 + q < nblocks ? part[(int64_t)(p0 + q) * E + at[i]] : 0.0;
#pragma unroll
      for (int q = 0; q < kBatch; ++q)
#pragma unroll
        for (int i = 0; i < kOwn; ++i) num::comp_add(s[i], c[i], val[q][i]);
    }
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      const int e = t + i * kFactorThreads;
      if (e < E) {
        const double val = s[i] + c[i];
        int a, b;
        unpack(e, a, b);
        if (a < F) {
          state[off_g(F) + a * F + b] = val;
          state[off_g(F) + b * F + a] = val;
          if (a == b) {
            sq[a * kSq + a] = s2 * val + v;
          } else {
            sq[a * kSq + b] = s2 * val;
            sq[b * kSq + a] = 0.0;
          }
        } else if (b < F) {
          state[off_c(F) + b] = val;
          sc[b] = val;
        } else {
          state[kYY] = val;
          ssum[0] = val;                                 // yy, until the scalars are formed
        }
      }
    }
  }
  __syncthreads();
  const double yy = ssum[0];
  // column j: the pivot, column j of L and row j of L^-1 (phase 1), then the rank-1 updates (phase 2), in which thread
  // (i, m) holds the entries x = m, m + kCols, ... of row i: all of them are loaded before the first is stored
  const int i = t / kCols, m = t - i * kCols;
  bool bad = false;
  for (int j = 0; j < F; ++j) {
    const double p = sq[j * kSq + j];
    if (!(p > 0.0) || !(p <= 1.79769313486231570815e308)) {          // (the same value in every thread)
      bad = true;
      break;
    }
    const double d = sqrt(p);
    if (t < F) {
      if (t != j) sq[t * kSq + j] = sq[t * kSq + j] / d;              // L[t][j] below the diagonal, L^-1[j][t] above it
      else sdg[j] = d, sxd[j] = 1.0 / d;
    }
    __syncthreads();
    if (i > j && i < F) {
      const double lij = sq[i * kSq + j];
      double cur[kPerRow], oth[kPerRow];
#pragma unroll
      for (int u = 0; u < kPerRow; ++u) {
        const int x = m + u * kCols;
        cur[u] = oth[u] = 0.0;
        if (x <= i) {
          cur[u] = x < j ? sq[x * kSq + i] : x == j ? 0.0 : sq[i * kSq + x];
          oth[u] = x == j ? sxd[j] : sq[x * kSq + j];
        }
      }
#pragma unroll
      for (int u = 0; u < kPerRow; ++u) {
        const int x = m + u * kCols;
        if (x <= i) {
          const double r = cur[u] - lij * oth[u];
          if (x <= j) sq[x * kSq + i] = r;                            // L^-1[i][x] -= L[i][j] L^-1[j][x]
          else sq[i * kSq + x] = r;                                   // A[i][x] -= L[i][j] L[x][j]
        }
      }
    }
    __syncthreads();
  }
  if (bad) {
    const double nan = num::qnan();
    if (t < kN && t != kYY) state[t] = nan;
    for (int k = t; k < F; k += kFactorThreads) state[off_b(F) + k] = nan;
    for (int k = t; k < F * F; k += kFactorThreads)
      state[off_linv(F) + k] = state[off_ainv(F) + k] = state[off_l(F) + k] = nan;
    if (t == 0) {
      state[kN] = (double)N;
      state[kF] = (double)F;
      for (int k = kF + 1; k < kScalars; ++k) state[k] = 0.0;
    }
    return;
  }
  auto X = [&](int a, int b) { return a == b ? sxd[a] : sq[b * kSq + a]; };       // L^-1[a][b], b <= a
  if (t < F) {                                           // w = L^-1 c
    double s = 0.0;
    for (int k = 0; k <= t; ++k) s += X(t, k) * sc[k];
    sw[t] = s;
    slog[t] = log(sdg[t]);
  }
  __syncthreads();
  if (t < F) {                                           // b = L^-T w; the squares of row t of L^-1
    double s = 0.0, r = 0.0;
    for (int k = t; k < F; ++k) s += X(k, t) * sw[k];
    for (int k = 0; k <= t; ++k) r += X(t, k) * X(t, k);
    sb[t] = s;
    srow[t] = r;
    state[off_b(F) + t] = s;
  }
  for (int idx = t; idx < F * F; idx += kFactorThreads) {      // A^-1 = L^-T L^-1, L^-1 and L
    const int a = idx / F, b = idx - a * F;
    if (b <= a) {
      double s = 0.0;
      for (int k = a; k < F; ++k) s += X(k, a) * X(k, b);
      state[off_ainv(F) + a * F + b] = s;
      state[off_ainv(F) + b * F + a] = s;
      state[off_linv(F) + idx] = X(a, b);
      state[off_l(F) + idx] = a == b ? sdg[a] : sq[a * kSq + b];
    } else {
      state[off_linv(F) + idx] = 0.0;
      state[off_l(F) + idx] = 0.0;
    }
  }
  __syncthreads();
  if ((t & 63) == 0 && t < 256) {                        // |w|^2 = c^T b, |b|^2, |L^-1|_F^2 = tr A^-1, sum log L_aa: four waves
    const int which = t >> 6;
    const double* __restrict__ src = which == 0 ? sw : which == 1 ? sb : which == 2 ? srow : slog;
    double s = 0.0;
    for (int k = 0; k < F; ++k) s += which >= 2 ? src[k] : src[k] * src[k];
    ssum[which] = s;
  }
  __syncthreads();
  if (t == 0) {
    const double quad = ssum[0], bb = ssum[1], tr = ssum[2], n = (double)N, nf = (double)(N - F), logdet = 2.0 * ssum[3];
    state[kLogLik] = -0.5 * (n * 1.83787706640934548356 + nf * log(v) + yy / v + logdet - (s2 / v) * quad);
    state[kDv] = -0.5 * (nf / v - yy / (v * v) + tr + (s2 / (v * v)) * quad + (s2 / v) * bb);
    state[kV] = v;
    state[kS2] = s2;
    state[kLogDet] = logdet;
    state[kQuad] = quad;
    state[kBB] = bb;
    state[kTrace] = tr;
    state[kN] = n;
    state[kF] = (double)F;
    for (int k = kF + 1; k < kScalars; ++k) state[k] = 0.0;
  }
}

// a tile of kRowTile rows of x [rows, F] as fp64; the rows beyond the end are zero
template <typename T>
__device__ __forceinline__ void stage_rows(const T* __restrict__ x, int64_t row0, int rows, int F, double* sx) {
  const T* __restrict__ src = x + row0 * F;
  for (int k = threadIdx.x; k < kRowTile * F; k += kThreads) {
    const int r = k / F;
    sx[r * kSq + (k - r * F)] = r < rows ? (double)src[k] : 0.0;
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void grad_kernel(const T* __restrict__ f, const T* __restrict__ y, int64_t N, int F,
                                                        const double* __restrict__ state, const T* __restrict__ upstream,
                                                        T* __restrict__ grad_f, double* __restrict__ grad_v) {
  __shared__ double sa[kMaxF * kSq];
  __shared__ double sx[kRowTile * kSq];
  __shared__ double sb[kMaxF];
  const int t = threadIdx.x, r = t / kLanes, m = t - r * kLanes;
  const double up = upstream ? (double)upstream[0] : 1.0;
  const double v = state[kV], s2 = state[kS2], ratio = s2 / v;
  if (blockIdx.x == 0 && t == 0 && grad_v) grad_v[0] = up * state[kDv];
  for (int k = t; k < F * F; k += kThreads) {
    const int a = k / F;
    sa[a * kSq + (k - a * F)] = state[off_ainv(F) + k];
  }
  if (t < F) sb[t] = state[off_b(F) + t];
  const int64_t tiles = (N + kRowTile - 1) / kRowTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRowTile;
    const int rows = (int)(N - row0 < kRowTile ? N - row0 : kRowTile);
    __syncthreads();
    stage_rows(f, row0, rows, F, sx);
    __syncthreads();
    if (r < rows) {
      const double* __restrict__ x = sx + r * kSq;
      double fb = 0.0;
      for (int k = 0; k < F; ++k) fb = fma(x[k], sb[k], fb);
      const double res = (double)y[row0 + r] - s2 * fb;
      T* __restrict__ out = grad_f + (row0 + r) * F;
      for (int a = m; a < F; a += kLanes) {
        const double* __restrict__ arow = sa + a * kSq;
        double s = 0.0;
        for (int k = 0; k < F; ++k) s = fma(arow[k], x[k], s);
        out[a] = (T)(up * ((ratio * res) * sb[a] - s2 * s));
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void predict_kernel(const T* __restrict__ fs, int64_t M, int F,
                                                           const double* __restrict__ state, double* __restrict__ mean,
                                                           double* __restrict__ var) {
  __shared__ double sl[kMaxF * kSq];
  __shared__ double sx[kRowTile * kSq];
  __shared__ double sb[kMaxF];
  __shared__ double sred[kRowTile][kLanes];
  const int t = threadIdx.x, r = t / kLanes, m = t - r * kLanes;
  const double v = state[kV], s2 = state[kS2];
  for (int k = t; k < F * F; k += kThreads) {
    const int a = k / F;
    sl[a * kSq + (k - a * F)] = state[off_linv(F) + k];
  }
  if (t < F) sb[t] = state[off_b(F) + t];
  const int64_t tiles = (M + kRowTile - 1) / kRowTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRowTile;
    const int rows = (int)(M - row0 < kRowTile ? M - row0 : kRowTile);
    __syncthreads();
    stage_rows(fs, row0, rows, F, sx);
    __syncthreads();
    const double* __restrict__ x = sx + r * kSq;
    double qsum = 0.0;
    for (int a = m; a < F; a += kLanes) {                // u_a = (L^-1 f*)_a, lane m adds u_a^2 for a = m, m + kLanes, ...
      const double* __restrict__ lrow = sl + a * kSq;
      double u = 0.0;
      for (int k = 0; k <= a; ++k) u = fma(lrow[k], x[k], u);
      qsum = fma(u, u, qsum);
    }
    sred[r][m] = qsum;
    __syncthreads();
    if (m == 0 && r < rows) {
      double fb = 0.0, qq = 0.0;
      for (int k = 0; k < F; ++k) fb = fma(x[k], sb[k], fb);
      for (int k = 0; k < kLanes; ++k) qq += sred[r][k];
      mean[row0 + r] = s2 * fb;
      var[row0 + r] = (v * s2) * qq + v;
    }
  }
}

}  // namespace raob

extern "C" int64_t sgmcmc_raob_workspace_doubles(int64_t N, int F) {
  if (!raob::sizes_ok(N, F)) return -1;
  return (int64_t)raob::blocks(N) * raob::part_doubles(F);
}

extern "C" int sgmcmc_raob_gram(const void* f, const void* y, int is_f64, int64_t N, int F, double* workspace,
                                void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!f || !y || !workspace || !raob::sizes_ok(N, F)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)raob::blocks(N)), block(raob::kThreads);
  if (is_f64) SGMCMC_LAUNCH(raob::gram_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)f,
                            (const double*)y, N, F, workspace);
  else SGMCMC_LAUNCH(raob::gram_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)f, (const float*)y, N, F,
                     workspace);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_raob_factor(const double* workspace, int64_t N, int F, double last_layer_var, double noise_var,
                                  const double* noise_var_device, double* state, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!workspace || !state || !raob::sizes_ok(N, F)) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(raob::factor_kernel, dim3(1), dim3(raob::kFactorThreads), 0, (hipStream_t)stream, workspace,
                raob::blocks(N), N, F, last_layer_var, noise_var, noise_var_device, state);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_raob_grad(const void* f, const void* y, int is_f64, int64_t N, int F, const double* state,
                                const void* upstream, void* grad_f, double* grad_noise_var, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!f || !y || !state || !grad_f || !raob::sizes_ok(N, F)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)raob::row_blocks(N)), block(raob::kThreads);
  if (is_f64) SGMCMC_LAUNCH(raob::grad_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)f,
                            (const double*)y, N, F, state, (const double*)upstream, (double*)grad_f, grad_noise_var);
  else SGMCMC_LAUNCH(raob::grad_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)f, (const float*)y, N, F,
                     state, (const float*)upstream, (float*)grad_f, grad_noise_var);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_raob_predict(const void* f_star, int is_f64, int64_t M, int F, const double* state, double* mean,
                                   double* var, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!f_star || !state || !mean || !var || !raob::sizes_ok(M, F)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)raob::row_blocks(M)), block(raob::kThreads);
  if (is_f64) SGMCMC_LAUNCH(raob::predict_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)f_star, M, F,
                            state, mean, var);
  else SGMCMC_LAUNCH(raob::predict_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)f_star, M, F, state,
                     mean, var);
  return (int)hipGetLastError();
}
