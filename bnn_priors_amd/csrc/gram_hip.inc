// The symmetric Gram walk on the fp64 matrix pipe, its shared pieces written once for corr_hip.inc and stein_hip.inc:
// G = M M^T of a matrix M [V rows][length], in 64 x 64 blocks of the upper triangle, the contraction split over
// workgroups.  Included from sgmcmc_hip.hip after numerics_hip.inc and before its users.
//
// Grid (pair_grid): x = block pair (bi, bj), bi <= bj, row-major over the upper triangle; y = split; z = the user's batch.
// Workgroup (pair, split) walks the chunks split, split + splits, ... of kChunk contracted elements (splits <= chunks:
// every workgroup has one) and stores its block into slab `split`; the user's next launch adds the slabs (slab_sums).
// Every sum's order is a function of (V, length, splits) alone.
// LDS: a tile of kTile rows x kChunk elements is staged as tile[row][k] in fp64 with row stride kRow = kChunk + 2 doubles:
// the 32 lanes of one ds_read_b64 group hold 16 rows x 2 k at double offsets 34 r + k = 2 r + k (mod 32), 32 bank pairs.
// v_mfma_f64_16x16x4_f64: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and receives
// D[i = (l >> 4) + 4 reg][j = l & 15], reg = 0 .. 3 (NOT the fp32 map; tests/test_weight_correlation.py's V = 17 and
// V = 65 cases would put 3 of 4 results in the wrong row otherwise).  A workgroup of 4 waves forms one 64 x 64 block,
// wave w the 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 MFMA tiles: 16 accumulated doubles per lane.
// lanczos::ritz_kernel (another shape, its own loop) uses the same lane map.

namespace gram {

static_assert(SGMCMC_CORR_TILE == SGMCMC_STEIN_TILE && SGMCMC_CORR_CHUNK == SGMCMC_STEIN_CHUNK, "one Gram geometry");
constexpr int kThreads = 256, kTile = SGMCMC_CORR_TILE, kChunk = SGMCMC_CORR_CHUNK;
constexpr int kRow = kChunk + 2;                        // LDS row stride in doubles (see above)
constexpr int kPerThread = kTile * kChunk / kThreads;   // elements of a tile a thread loads
static_assert(kTile == 64 && kChunk % 4 == 0 && kPerThread * kThreads == kTile * kChunk, "tile geometry");
static_assert(kThreads % kTile == 0 && kThreads % kChunk == 0 && kChunk <= 64, "loader geometry");
typedef double f64x4 __attribute__((ext_vector_type(4)));

inline int tiles_of(int V) { return (V + kTile - 1) / kTile; }
inline int pairs_of(int V) { return tiles_of(V) * (tiles_of(V) + 1) / 2; }
inline int64_t chunks_of(int64_t length) { return (length + kChunk - 1) / kChunk; }
// workgroups that share the chunks of one block pair: enough to fill target_blocks, no more than the workspace has slabs
inline int splits(int V, int64_t length, int64_t workspace_bytes, int max_splits, int target_blocks) {
  int64_t s = chunks_of(length);
  if (s > max_splits) s = max_splits;
  if (s > target_blocks / pairs_of(V)) s = target_blocks / pairs_of(V);
  if (s > workspace_bytes / ((int64_t)sizeof(double) * V * V)) s = workspace_bytes / ((int64_t)sizeof(double) * V * V);
  return (int)(s < 0 ? 0 : s);
}
inline dim3 pair_grid(int V, int splits, int batch = 1) { return dim3(pairs_of(V), splits, batch); }

// The Gram kernels themselves stay with each user, text and all: written with shared device helpers they compile to other
// code (docs/lab_notes.md).

// s[e] = sum_q slabs[q stride + at[e]] from 0 in ascending q; reading (i, j) at min V + max mirrors the triangle
template <int N>
__device__ __forceinline__ void slab_sums(const double* __restrict__ slabs, int splits, size_t stride, const size_t (&at)[N],
                                          double (&s)[N]) {
#pragma unroll
  for (int e = 0; e < N; ++e) s[e] = 0.0;
  for (int q = 0; q < splits; ++q) {
    const double* slab = slabs + (size_t)q * stride;
#pragma unroll
    for (int e = 0; e < N; ++e) s[e] += slab[at[e]];
  }
}

}  // namespace gram
