// mlp_hip.inc -- fused forward + backward of the BASELINE dense classifier
// (ClassificationDenseNet: Linear-ReLU-Linear-ReLU-Linear + categorical likelihood;
//  reference: bnn_priors/models/dense_nets.py:48-67, models/base.py:168-191) for gfx950.
//
// Why: one leapfrog step of this net is ~30 ATen/rocBLAS launches of a few microseconds
// each (three GEMMs forward, five backward, bias/ReLU/softmax/NLL kernels, reductions); at
// batch 128 x 42k parameters the step is pure launch latency.  This kernel does the whole
// stochastic-gradient evaluation of -(1/B) sum_i log p(y_i | x_i) in ONE launch:
//
//   grid  = ceil(B / 16) workgroups, each owns 16 batch rows (gathered through an index
//           array, so the minibatch is never materialised);
//   block = 1024 threads = 16 wavefronts; every contraction runs on the matrix cores with
//           v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: bit-for-bit an fmaf chain, so
//           no precision is given up); the two 784-wide contractions are spread over all 16
//           waves (K quarters x column tiles), the small layers use 4;
//   LDS   = the 16 x IN input slice (50 KB for MNIST), activations and their gradients;
//   out   = per-workgroup PARTIAL parameter gradients gpart[s][D] (packed, 4-aligned per
//           tensor like the sampler's noise index), per-workgroup loss / #correct.
// The partials are summed over s in a fixed order by sgmcmc_grad_reduce_prior (no atomics:
// run-to-run bitwise reproducible), which also adds the prior's gradient.
//
// Two kernel families run the same arithmetic: the one-launch kernel above (mlp_fwdbwd_body: 1024 threads, dynamic LDS)
// and the two-launch split of the latency-critical leapfrog step (mlp_f1_body + mlp_rest_body: 256 threads, static LDS,
// KSPLIT x more workgroups; further down).  Every phase -- forward 1's load block and MFMA chain, the layer-1 combine,
// forward 2 / 3, the softmax cross-entropy, the dW3 / d2 / dW2 / d1 tiles, the bias sums, the dW1 tile pair with its
// transposed store -- is ONE __device__ function on a struct of LDS pointers (MlpLds); a body decides which waves run
// it, stages its arrays (the dynamic carve-up; the split's register-staged global loads) and places the barriers.  So
// the routes give the same bits wherever a K quarter has at most F1_UNROLL steps
// (tests/test_dense_step_reference.py::test_routes_agree_bit_for_bit).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sgmcmc_hip.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMlpThreads = 1024;   // 16 wavefronts: the first layer's K and tiles are spread over them
constexpr int kMlpWaves = kMlpThreads / 64;
constexpr int KSPLIT = 4;         // K quarters of forward 1 / column-tile stride of backward 1
constexpr int F1_UNROLL = 13;     // >= ceil(49 / KSPLIT): a wave issues all its W1 loads at once for IN = 784
constexpr int STG = 20;           // row stride of the per-wave 16x16 store-staging patch
constexpr int ROWS = SGMCMC_MLP_ROWS;  // batch rows per workgroup (one MFMA M tile)
constexpr int HP = 64;                 // hidden widths are padded to 4 MFMA column tiles
constexpr int HS = HP + 4;             // LDS row stride of the [ROWS][HP] activation arrays
constexpr int OP = 16;                 // output width padded to one tile

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

struct IdxBlock { int32_t idx[SGMCMC_MLP_MAX_INLINE]; };

// ---------------------------------------------------------------- the phases, each written once
// Both kernel families run these.  A phase is the arithmetic of one wave (or one thread) on the workgroup's LDS arrays;
// WHO runs it (which waves, which workgroup of a slice), the barriers between phases and how the arrays were staged are
// the caller's.  The library is built with -ffp-contract=off, so the order of operations written here is the result's
// bits on every route: j ascending in every MFMA chain, acc0 / acc1 alternating in forward 1, rows ascending in the sums.
// (r, g) = (lane & 15, lane >> 4) are the MFMA fragment coordinates, nt / mt a 16-wide column / row tile.
struct MlpLds {
  float *h1s, *h2s;  // [ROWS][HS]  relu(layer 1), relu(layer 2)
  float *d1s, *d2s;  // [ROWS][HS]  dL/d(pre-activation 1), dL/d(pre-activation 2)
  float *lgs, *dfs;  // [ROWS][OP]  logits, dL/dlogits
  float* red;        // [2][ROWS]   per-row loss / correct
  float *w2s, *w3s;  // [HP][HS], [OP][HS]  W2, W3, zero padded
  float* bs;         // [3][HP]     b1, b2, b3 (zero padded)
  int* ys;           // [ROWS]      labels (-1 = padding row)
  float* patch;      // [16][STG]   THIS wave's store-staging patch
};

// forward 1, one block of <= F1_UNROLL K steps from step jb on, in two halves so that a caller can put its own staging
// between them: every W1 load of the lane is issued (W1 was just rewritten by the sampler kernel on other XCDs: these
// are long-latency reads) ...
__device__ __forceinline__ void mlp_f1_load(float4 (&w)[F1_UNROLL], const float* __restrict__ wrow, bool live, int jb,
                                            int j1, int g, int IN) {
#pragma unroll
  for (int u = 0; u < F1_UNROLL; ++u) {
    const int k = 16 * (jb + u) + 4 * g;
    w[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && jb + u < j1 && k < IN) w[u] = *reinterpret_cast<const float4*>(wrow + k);
  }
}
// ... then the MFMA chain on two accumulators; xrow: this lane's four inputs of step jb (row r, columns 16 jb + 4 g ..)
__device__ __forceinline__ void mlp_f1_chain(const float4 (&w)[F1_UNROLL], const float* xrow, int jb, int j1,
                                             f32x4& acc0, f32x4& acc1) {
#pragma unroll
  for (int u = 0; u < F1_UNROLL; ++u) {
    if (jb + u < j1) {
      const float4 a = *reinterpret_cast<const float4*>(xrow + 16 * u);
      acc0 = mfma4(a.x, w[u].x, acc0);
      acc1 = mfma4(a.y, w[u].y, acc1);
      acc0 = mfma4(a.z, w[u].z, acc0);
      acc1 = mfma4(a.w, w[u].w, acc1);
    }
  }
}

// h1[row][n] = relu(b1 + the four K-quarter partials, in this order)
__device__ __forceinline__ void mlp_combine1(const MlpLds& S, int H1, int row, int n, float q0, float q1, float q2,
                                             float q3) {
  float pre = S.bs[n];
  pre += q0;
  pre += q1;
  pre += q2;
  pre += q3;
  S.h1s[row * HS + n] = (n < H1 && pre > 0.f) ? pre : 0.f;
}

// forward 2: h2 = relu(h1 W2^T + b2), column tile nt
__device__ __forceinline__ void mlp_forward2(const MlpLds& S, int H2, int nt, int r, int g) {
  const int n = 16 * nt + r;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < HP / 4; ++j) {
    const int k = 4 * j + g;
    acc = mfma4(S.h1s[r * HS + k], S.w2s[n * HS + k], acc);
  }
  const float bias = S.bs[HP + n];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float pre = acc[i] + bias;
    S.h2s[(4 * g + i) * HS + n] = (n < H2 && pre > 0.f) ? pre : 0.f;
  }
}

// forward 3: logits = h2 W3^T + b3 (one tile)
__device__ __forceinline__ void mlp_forward3(const MlpLds& S, int r, int g) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < HP / 4; ++j) {
    const int k = 4 * j + g;
    acc = mfma4(S.h2s[r * HS + k], S.w3s[r * HS + k], acc);
  }
  const float bias = S.bs[2 * HP + r];
#pragma unroll
  for (int i = 0; i < 4; ++i) S.lgs[(4 * g + i) * OP + r] = acc[i] + bias;
}

// softmax cross-entropy, mean over the FULL batch (models/base.py:57-62,181-182):
//   loss_i = logsumexp(f_i) - f_i[y_i];  dL/df = (softmax - onehot) / B.
// Thread t of 256 owns logit (row, c) = (t >> 4, t & 15); 16-lane groups reduce with shuffles.
__device__ __forceinline__ void mlp_softmax_ce(const MlpLds& S, int OUT, float st, float invB, int t) {
  const int row = t >> 4, c = t & 15;
  const int y = S.ys[row];
  const float v = c < OUT ? S.lgs[row * OP + c] * st : -INFINITY;
  float m = v;
  int arg = c;
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off, 16);
    const int oa = __shfl_xor(arg, off, 16);
    if (om > m || (om == m && oa < arg)) { m = om; arg = oa; }  // first maximal index
  }
  float se = c < OUT ? expf(v - m) : 0.f;
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) se += __shfl_xor(se, off, 16);
  const float lse = m + logf(se);
  float d = 0.f;
  if (y >= 0 && c < OUT) d = (expf(v - lse) - (c == y ? 1.f : 0.f)) * invB * st;
  S.dfs[row * OP + c] = d;
  if (c == 0) {
    S.red[row] = y >= 0 ? lse - S.lgs[row * OP + y] * st : 0.f;
    S.red[ROWS + row] = (y >= 0 && arg == y) ? 1.f : 0.f;
  }
}
// ... and the slice's loss / #correct, rows ascending (one thread)
__device__ __forceinline__ void mlp_loss_sums(const MlpLds& S, float* loss, float* correct) {
  float l = 0.f, c = 0.f;
  for (int i = 0; i < ROWS; ++i) { l += S.red[i]; c += S.red[ROWS + i]; }
  *loss = l;
  *correct = c;
}

// a bias gradient: column `col` of a [ROWS][stride] array summed over the rows, ascending
__device__ __forceinline__ float mlp_column_sum(const float* a, int stride, int col) {
  float s = 0.f;
  for (int i = 0; i < ROWS; ++i) s += a[i * stride + col];
  return s;
}

// the A fragments of a weight-gradient tile: d^T for row tile m0 of d1s / d2s, one value per K step (4 batch rows)
__device__ __forceinline__ void mlp_dT_fragment(float (&a)[ROWS / 4], const float* d, int m0, int r, int g) {
#pragma unroll
  for (int j = 0; j < ROWS / 4; ++j) a[j] = d[(4 * j + g) * HS + m0 + r];
}

// backward 3: dW3 = df^T h2, column tile nt
__device__ __forceinline__ void mlp_dW3_tile(const MlpLds& S, float* __restrict__ gW3, int OUT, int H2, int nt, int r,
                                             int g) {
  const int n = 16 * nt + r;  // h2 unit
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < ROWS / 4; ++j) {
    const int k = 4 * j + g;  // batch row
    acc = mfma4(S.dfs[k * OP + r], S.h2s[k * HS + n], acc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = 4 * g + i;  // output class
    if (m < OUT && n < H2) gW3[m * H2 + n] = acc[i];
  }
}
// ... and d2 = (df W3) * [h2 > 0], column tile nt
__device__ __forceinline__ void mlp_backward3_d2(const MlpLds& S, int nt, int r, int g) {
  const int n = 16 * nt + r;
  f32x4 dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < OP / 4; ++j) {
    const int k = 4 * j + g;  // class
    dacc = mfma4(S.dfs[r * OP + k], S.w3s[k * HS + n], dacc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 4 * g + i;
    S.d2s[row * HS + n] = S.h2s[row * HS + n] > 0.f ? dacc[i] : 0.f;
  }
}

// backward 2: dW2 = d2^T h1, tile (row tile m0 whose fragments are `a`, column tile nt)
__device__ __forceinline__ void mlp_dW2_tile(const MlpLds& S, const float (&a)[ROWS / 4], float* __restrict__ gW2,
                                             int H1, int H2, int m0, int nt, int r, int g) {
  const int n = 16 * nt + r;  // h1 unit
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < ROWS / 4; ++j) acc = mfma4(a[j], S.h1s[(4 * j + g) * HS + n], acc);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + 4 * g + i;
    if (m < H2 && n < H1) gW2[m * H1 + n] = acc[i];
  }
}
// ... and d1 = (d2 W2) * [h1 > 0], column tile nt
__device__ __forceinline__ void mlp_backward2_d1(const MlpLds& S, int nt, int r, int g) {
  const int n = 16 * nt + r;
  f32x4 dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < HP / 4; ++j) {
    const int k = 4 * j + g;  // h2 unit
    dacc = mfma4(S.d2s[r * HS + k], S.w2s[k * HS + n], dacc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 4 * g + i;
    S.d1s[row * HS + n] = S.h1s[row * HS + n] > 0.f ? dacc[i] : 0.f;
  }
}

// backward 1: dW1 = d1^T x for row tile m0 (fragments `a`) and the input-column tiles t0 and, if `two`, t1 of the
// [ROWS][xstride] slice xs, whose column 0 is input column col0.  Each 16x16 result is transposed through the wave's LDS
// patch so that the store is one 16-byte access per lane (4 lanes cover a 64-byte row segment).
__device__ __forceinline__ void mlp_dW1_pair(const MlpLds& S, const float (&a)[ROWS / 4], const float* xs, int xstride,
                                             int t0, int t1, bool two, int col0, float* __restrict__ gW1, int H1, int IN,
                                             int m0, int lane) {
  const int r = lane & 15, g = lane >> 4;
  const int srow = lane >> 2, sc4 = (lane & 3) * 4;  // this lane's row / column group in the patch
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < ROWS / 4; ++j) {
    const float* xr = xs + (4 * j + g) * xstride;
    acc0 = mfma4(a[j], xr[16 * t0 + r], acc0);
    if (two) acc1 = mfma4(a[j], xr[16 * t1 + r], acc1);
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (half == 1 && !two) break;
    const f32x4 acc = half ? acc1 : acc0;
    const int nb = col0 + 16 * (half ? t1 : t0);
#pragma unroll
    for (int i = 0; i < 4; ++i) S.patch[(4 * g + i) * STG + r] = acc[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float4 v = *reinterpret_cast<const float4*>(S.patch + srow * STG + sc4);
    const int m = m0 + srow, col = nb + sc4;
    if (m < H1 && col < IN) *reinterpret_cast<float4*>(gW1 + (int64_t)m * IN + col) = v;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------- the one-launch kernel
template <bool INLINE>
__device__ __forceinline__ void mlp_fwdbwd_body(const sgmcmc_mlp_args& P, const IdxBlock* IB) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int IN = P.in_features, H1 = P.hidden1, H2 = P.hidden2, OUT = P.out_features;
  const int INp = (IN + 15) & ~15;  // K of the first layer, padded to 16
  const int XS = INp + 4;           // LDS row stride of the input slice (bank spread)
  float* xs = reinterpret_cast<float*>(smem_raw);  // [ROWS][XS]
  float* h1s = xs + ROWS * XS;                     // [ROWS][HS]  relu(layer 1)
  float* h2s = h1s + ROWS * HS;                    // [ROWS][HS]  relu(layer 2)
  float* d1s = h2s + ROWS * HS;                    // [ROWS][HS]  dL/d(pre-activation 1)
  float* d2s = d1s + ROWS * HS;                    // [ROWS][HS]  dL/d(pre-activation 2)
  float* lgs = d2s + ROWS * HS;                    // [ROWS][OP]  logits
  float* dfs = lgs + ROWS * OP;                    // [ROWS][OP]  dL/dlogits
  float* red = dfs + ROWS * OP;                    // [2][ROWS]   per-row loss / correct
  float* w2s = red + 2 * ROWS;                     // [HP][HS]    W2, zero padded
  float* w3s = w2s + HP * HS;                      // [OP][HS]    W3, zero padded
  float* bs = w3s + OP * HS;                       // [3][HP]     b1, b2, b3 (zero padded)
  float* f1p = bs + 3 * HP;                        // [KSPLIT][ROWS][HS] K-split partials of layer 1
  float* stg = f1p + KSPLIT * ROWS * HS;           // [kWaves][16][STG] per-wave store staging
  int64_t* rowp = reinterpret_cast<int64_t*>(stg + kMlpWaves * 16 * STG);  // [ROWS] source row or -1
  int* ys = reinterpret_cast<int*>(rowp + ROWS);   // [ROWS] labels (-1 = padding row)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;  // MFMA fragment coordinates
  const MlpLds lds = {h1s, h2s, d1s, d2s, lgs, dfs, red, w2s, w3s, bs, ys, stg + wave * 16 * STG};
  const int slice = blockIdx.x;
  const int row0 = slice * ROWS;
  float* __restrict__ gp = P.gpart + (int64_t)slice * P.gpart_stride;
  const float invB = P.grad_scale > 0.f ? P.grad_scale : 1.0f / (float)P.batch;
  int tp = 0;
#define MLP_TRACE() do { if (P.trace && blockIdx.x == 0 && tid == 0) P.trace[tp] = (int64_t)clock64(); ++tp; } while (0)
  MLP_TRACE();

  // ---- phase 0a: resolve the 16 row indices / labels; stage the small weights and biases
  if (P.args_src && blockIdx.x == 0 && tid < (P.args_bytes >> 2))
    reinterpret_cast<uint32_t*>(P.args_dst)[tid] = reinterpret_cast<const uint32_t*>(P.args_src)[tid];
  if (tid < ROWS) {
    const int b = row0 + tid;
    int64_t src = -1;
    if (b < P.batch) src = INLINE ? (int64_t)IB->idx[b] : (P.idx ? P.idx[b] : (int64_t)b);
    rowp[tid] = src;
    ys[tid] = src >= 0 ? (int)P.Y[src] : -1;
  }
  for (int e = tid; e < HP * HS; e += kMlpThreads) {
    const int m = e / HS, k = e - m * HS;
    w2s[e] = (m < H2 && k < H1) ? P.W2[m * H1 + k] : 0.f;
  }
  for (int e = tid; e < OP * HS; e += kMlpThreads) {
    const int m = e / HS, k = e - m * HS;
    w3s[e] = (m < OUT && k < H2) ? P.W3[m * H2 + k] : 0.f;
  }
  if (tid < HP) {
    bs[tid] = tid < H1 ? P.b1[tid] : 0.f;
    bs[HP + tid] = tid < H2 ? P.b2[tid] : 0.f;
    bs[2 * HP + tid] = tid < OUT ? P.b3[tid] : 0.f;
  }
  __syncthreads();
  // ---- phase 0b: gather the 16 input rows into LDS; every thread's loads are independent
  {
    const int n4 = INp >> 2, in4 = IN >> 2;  // IN % 4 == 0 is checked by the host
    const int total = ROWS * n4;
    for (int e = tid; e < total; e += kMlpThreads) {
      const int rr = e / n4, c = e - rr * n4;
      const int64_t src = rowp[rr];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (src >= 0 && c < in4) v = *reinterpret_cast<const float4*>(P.X + src * (int64_t)IN + 4 * c);
      *reinterpret_cast<float4*>(xs + rr * XS + 4 * c) = v;
    }
  }
  __syncthreads();
  MLP_TRACE();  // end of phase0

  // ---- forward 1: h1 = relu(x W1^T + b1).  Wave (nt, q): hidden units 16nt..16nt+15, K quarter q (partials in f1p)
  {
    const int nt = wave & 3, q = wave >> 2;
    const int n = 16 * nt + r;
    const float* __restrict__ wrow = P.W1 + (int64_t)(n < H1 ? n : 0) * IN;
    const bool live = n < H1;
    const int steps = INp >> 4;
    const int j0 = (steps * q) / KSPLIT, j1 = (steps * (q + 1)) / KSPLIT;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int jb = j0; jb < j1; jb += F1_UNROLL) {
      float4 b[F1_UNROLL];
      mlp_f1_load(b, wrow, live, jb, j1, g, IN);
      mlp_f1_chain(b, xs + r * XS + 16 * jb + 4 * g, jb, j1, acc0, acc1);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) f1p[(q * ROWS + 4 * g + i) * HS + n] = acc0[i] + acc1[i];
  }
  __syncthreads();
  for (int e = tid; e < ROWS * HP; e += kMlpThreads) {
    const int row = e / HP, n = e - row * HP;
    const float* part = f1p + row * HS + n;
    mlp_combine1(lds, H1, row, n, part[0], part[ROWS * HS], part[2 * ROWS * HS], part[3 * ROWS * HS]);
  }
  __syncthreads();
  MLP_TRACE();  // end of f1

  // ---- forward 2 (waves 0-3, one column tile each), forward 3 (one tile: wave 0)
  if (wave < 4) mlp_forward2(lds, H2, wave, r, g);
  __syncthreads();
  MLP_TRACE();  // end of f2
  if (wave == 0) mlp_forward3(lds, r, g);
  __syncthreads();
  MLP_TRACE();  // end of f3

  // ---- softmax cross-entropy: the first 256 threads own one logit each
  if (tid < ROWS * OP) mlp_softmax_ce(lds, OUT, P.inv_softmax_temp, invB, tid);
  __syncthreads();
  if (tid == 0) mlp_loss_sums(lds, P.loss_part + slice, P.correct_part + slice);
  MLP_TRACE();  // end of softmax

  // ---- backward 3: dW3 and d2 (waves 0-3, one column tile each), db3 (wave 4)
  if (wave < 4) {
    mlp_dW3_tile(lds, gp + P.off_W3, OUT, H2, wave, r, g);
    mlp_backward3_d2(lds, wave, r, g);
  } else if (wave == 4 && lane < OUT) {
    gp[P.off_b3 + lane] = mlp_column_sum(dfs, OP, lane);
  }
  __syncthreads();
  MLP_TRACE();  // end of b3

  // ---- backward 2: dW2 (16 tiles: one per wave), d1 (waves 0-3), db2 (wave 4)
  {
    float a[ROWS / 4];
    mlp_dT_fragment(a, d2s, 16 * (wave & 3), r, g);
    mlp_dW2_tile(lds, a, gp + P.off_W2, H1, H2, 16 * (wave & 3), wave >> 2, r, g);
  }
  if (wave < 4) {
    mlp_backward2_d1(lds, wave, r, g);
  } else if (wave == 4 && lane < H2) {
    gp[P.off_b2 + lane] = mlp_column_sum(d2s, HS, lane);
  }
  __syncthreads();
  MLP_TRACE();  // end of b2

  // ---- backward 1: dW1.  Wave (mt, c): hidden-unit tile mt, input-column tiles c, c+4, c+8, ... two at a time;
  //      db1 (wave 4)
  {
    const int m0 = 16 * (wave & 3), tiles = INp >> 4;
    float a[ROWS / 4];
    mlp_dT_fragment(a, d1s, m0, r, g);
    for (int t = wave >> 2; t < tiles; t += 2 * KSPLIT)
      mlp_dW1_pair(lds, a, xs, XS, t, t + KSPLIT, t + KSPLIT < tiles, 0, gp + P.off_W1, H1, IN, m0, lane);
    if (wave == 4 && lane < H1) gp[P.off_b1 + lane] = mlp_column_sum(d1s, HS, lane);
  }
  if (P.trace) __syncthreads();
  MLP_TRACE();  // end of b1
#undef MLP_TRACE
}

__global__ __launch_bounds__(kMlpThreads) void mlp_fwdbwd_kernel(sgmcmc_mlp_args P) {
  mlp_fwdbwd_body<false>(P, nullptr);
}
// FIN: the LAST workgroup (blockIdx.x == number of slices) runs the deferred per-segment
// bookkeeping of the previous transition instead of a batch slice
__global__ __launch_bounds__(kMlpThreads) void mlp_fwdbwd_kernel_inline(sgmcmc_mlp_args P, IdxBlock IB) {
  mlp_fwdbwd_body<true>(P, &IB);
}
__global__ __launch_bounds__(kMlpThreads) void mlp_fwdbwd_kernel_inline_fin(sgmcmc_mlp_args P, IdxBlock IB,
                                                                            sgmcmc_layout L,
                                                                            sgmcmc_step_args Aprev) {
  const int slices = (P.batch + ROWS - 1) / ROWS;
  if ((int)blockIdx.x == slices) { finalize_small_body(L, Aprev); return; }
  mlp_fwdbwd_body<true>(P, &IB);
}

}  // namespace

extern "C" {

int64_t sgmcmc_mlp_lds_bytes(int in_features) {
  const int INp = (in_features + 15) & ~15;
  return (int64_t)sizeof(float) * (ROWS * (INp + 4) + 4 * ROWS * HS + 2 * ROWS * OP + 2 * ROWS +
                                   HP * HS + OP * HS + 3 * HP + KSPLIT * ROWS * HS +
                                   kMlpWaves * 16 * STG) +
         (int64_t)sizeof(int64_t) * ROWS + (int64_t)sizeof(int) * ROWS;
}

namespace {
// the shapes the kernels are written for (batch bounds are each entry point's own); `split`: a K quarter of the first
// layer must also fit the F1_UNROLL steps the two-launch split keeps in registers
bool dense_shape_ok(const sgmcmc_mlp_args& m, bool split = false) {
  if (m.batch <= 0 || m.in_features <= 0 || (m.in_features & 3) || m.hidden1 <= 0 || m.hidden1 > HP ||
      m.hidden2 <= 0 || m.hidden2 > HP || m.out_features <= 0 || m.out_features > OP ||
      sgmcmc_mlp_lds_bytes(m.in_features) > 160 * 1024)
    return false;
  const int steps16 = ((m.in_features + 15) & ~15) >> 4;
  return !split || (steps16 + KSPLIT - 1) / KSPLIT <= F1_UNROLL;
}

// raise the dynamic-LDS limit of `kernels` to `lds` bytes when that is above `granted`, the caller's high-water mark
// (ask for what is needed: static LDS counts against the same 160 KiB)
hipError_t grant_dynamic_lds(std::initializer_list<const void*> kernels, int64_t lds, int64_t& granted) {
  if (lds <= granted) return hipSuccess;
  for (const void* k : kernels) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  granted = lds;
  return hipSuccess;
}

sgmcmc_grad_parts grad_parts_of(const sgmcmc_mlp_args& mlp, double num_data) {
  sgmcmc_grad_parts G;
  G.gpart = mlp.gpart; G.loss_part = mlp.loss_part; G.correct_part = mlp.correct_part;
  G.stride = mlp.gpart_stride; G.num_data = num_data; G.n_slices = (mlp.batch + ROWS - 1) / ROWS; G.batch = mlp.batch;
  return G;
}
}  // namespace

int sgmcmc_mlp_fwdbwd(const sgmcmc_mlp_args* P, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!P || !dense_shape_ok(*P)) return (int)hipErrorInvalidValue;
  const int64_t lds = sgmcmc_mlp_lds_bytes(P->in_features);
  static int64_t granted = 0;
  const hipError_t e = grant_dynamic_lds({reinterpret_cast<const void*>(mlp_fwdbwd_kernel)}, lds, granted);
  if (e != hipSuccess) return (int)e;
  const int slices = (P->batch + ROWS - 1) / ROWS;
  SGMCMC_LAUNCH(mlp_fwdbwd_kernel, dim3((unsigned)slices), dim3(kMlpThreads), (size_t)lds,
                     (hipStream_t)stream, *P);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- two-launch split
// The single-launch kernel is bounded by what ONE CU can pull / push per 16-row slice (157 KB of
// W1 in, 157 KB of dW1 out).  For the latency-critical leapfrog step the two 784-wide phases are
// spread over KSPLIT x more workgroups, with no in-kernel synchronisation between workgroups:
//   K1 mlp_f1_kernel   (slices x KSPLIT WGs): gather a K quarter of the slice's rows, partial
//                      x W1^T -> h1part (global); stash the gathered quarter for K2
//   K2 mlp_rest_kernel (slices x KSPLIT WGs): every WG of a slice recomputes the (tiny) middle --
//                      combine partials, layers 2/3, softmax-CE, backward 3/2 -> d1 -- and then
//                      produces the dW1 tiles of ITS quarter of the input columns; the q = 0 WG
//                      also writes the small gradients and the loss.
namespace {
constexpr int kSplitThreads = 256;
constexpr int XQ = 16 * F1_UNROLL;  // columns of one K quarter (<= 208)
constexpr int XQS = XQ + 4;         // LDS row stride

struct SplitScratch {
  float* h1part;  // [slices][KSPLIT][ROWS][HP]
  float* xq;      // [slices][KSPLIT][ROWS][XQ]
  int* ys;        // [slices][ROWS]
};
__device__ __forceinline__ SplitScratch split_scratch(const sgmcmc_mlp_args& P) {
  const int64_t slices = (P.batch + ROWS - 1) / ROWS;
  SplitScratch S;
  S.h1part = P.split_scratch;
  S.xq = S.h1part + slices * KSPLIT * ROWS * HP;
  S.ys = reinterpret_cast<int*>(S.xq + slices * KSPLIT * ROWS * XQ);
  return S;
}

// blockIdx.x = slice * KSPLIT + q; the data-set row of batch row b is idx32[b], or idx16[b] when idx32 is null
__device__ __forceinline__ void mlp_f1_body(const sgmcmc_mlp_args& P, const int32_t* idx32, const uint16_t* idx16) {
  __shared__ __attribute__((aligned(16))) float xs[ROWS * XQS];
  __shared__ int64_t rowp[ROWS];
  const int IN = P.in_features, H1 = P.hidden1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int slice = blockIdx.x / KSPLIT, q = blockIdx.x % KSPLIT;
  const int steps = ((IN + 15) & ~15) >> 4;
  const int j0 = (steps * q) / KSPLIT, j1 = (steps * (q + 1)) / KSPLIT;  // <= F1_UNROLL (host checks)
  const int c0 = 16 * j0, qw = 16 * (j1 - j0);
  const SplitScratch S = split_scratch(P);
  if (tid < ROWS) {
    const int b = slice * ROWS + tid;
    const int64_t src = b < P.batch ? (idx32 ? (int64_t)idx32[b] : (int64_t)idx16[b]) : -1;
    rowp[tid] = src;
    if (q == 0) S.ys[slice * ROWS + tid] = src >= 0 ? (int)P.Y[src] : -1;
  }
  __syncthreads();
  // gather first (oldest loads), then this lane's W1 slice; the gather is consumed first
  const int q4 = qw >> 2;
  constexpr int XG = (ROWS * (XQ / 4) + kSplitThreads - 1) / kSplitThreads;  // 4
  float4 xg[XG];
#pragma unroll
  for (int u = 0; u < XG; ++u) {
    const int e = tid + u * kSplitThreads;
    xg[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < ROWS * q4) {
      const int rr = e / q4, c = e - rr * q4;
      const int64_t src = rowp[rr];
      if (src >= 0 && c0 + 4 * c < IN) xg[u] = *reinterpret_cast<const float4*>(P.X + src * (int64_t)IN + c0 + 4 * c);
    }
  }
  const int n = 16 * wave + r;
  const bool live = n < H1;
  const float* __restrict__ wrow = P.W1 + (int64_t)(live ? n : 0) * IN;
  float4 w[F1_UNROLL];
  mlp_f1_load(w, wrow, live, j0, j1, g, IN);
  float* __restrict__ xq = S.xq + ((int64_t)(slice * KSPLIT + q) * ROWS) * XQ;
#pragma unroll
  for (int u = 0; u < XG; ++u) {
    const int e = tid + u * kSplitThreads;
    if (e < ROWS * q4) {
      const int rr = e / q4, c = e - rr * q4;
      *reinterpret_cast<float4*>(xs + rr * XQS + 4 * c) = xg[u];
      *reinterpret_cast<float4*>(xq + rr * XQ + 4 * c) = xg[u];
    }
  }
  __syncthreads();
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  mlp_f1_chain(w, xs + r * XQS + 4 * g, j0, j1, acc0, acc1);
  float* __restrict__ hp = S.h1part + ((int64_t)(slice * KSPLIT + q) * ROWS) * HP;
#pragma unroll
  for (int i = 0; i < 4; ++i) hp[(4 * g + i) * HP + n] = acc0[i] + acc1[i];
}

__global__ __launch_bounds__(kSplitThreads) void mlp_f1_kernel(sgmcmc_mlp_args P, IdxBlock IB) {
  mlp_f1_body(P, IB.idx, nullptr);
}

// blockIdx.x = slice * KSPLIT + q ; one EXTRA trailing block runs the deferred finalize of the
// previous transition (it has the whole kernel's duration to do so)
__device__ __forceinline__ void mlp_rest_body(const sgmcmc_mlp_args& P, const sgmcmc_layout& L,
                                              const sgmcmc_step_args& Aprev, int with_finalize) {
  if ((int)blockIdx.x == ((P.batch + ROWS - 1) / ROWS) * KSPLIT) {
    if (with_finalize) finalize_small_body(L, Aprev);
    return;
  }
  __shared__ __attribute__((aligned(16))) float xs[ROWS * XQS];
  __shared__ float h1s[ROWS * HS], h2s[ROWS * HS], d1s[ROWS * HS], d2s[ROWS * HS];
  __shared__ float lgs[ROWS * OP], dfs[ROWS * OP], red[2 * ROWS];
  __shared__ float w2s[HP * HS], w3s[OP * HS], bs[3 * HP];
  __shared__ __attribute__((aligned(16))) float stg[(kSplitThreads / 64) * 16 * STG];
  __shared__ int ys[ROWS];
  const int IN = P.in_features, H1 = P.hidden1, H2 = P.hidden2, OUT = P.out_features;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int slice = blockIdx.x / KSPLIT, q = blockIdx.x % KSPLIT;
  const int steps = ((IN + 15) & ~15) >> 4;
  const int j0 = (steps * q) / KSPLIT, j1 = (steps * (q + 1)) / KSPLIT;
  const int c0 = 16 * j0, qw = 16 * (j1 - j0);
  const SplitScratch S = split_scratch(P);
  float* __restrict__ gp = P.gpart + (int64_t)slice * P.gpart_stride;
  const float invB = P.grad_scale > 0.f ? P.grad_scale : 1.0f / (float)P.batch;
  const bool lead = q == 0;  // writes the small gradients and the loss of the slice
  const MlpLds lds = {h1s, h2s, d1s, d2s, lgs, dfs, red, w2s, w3s, bs, ys, stg + wave * 16 * STG};

  // ---- all input loads up front, in registers: K1's partials, the stashed x quarter, W2, W3
  constexpr int HPN = ROWS * HP / kSplitThreads;                                // 4
  float hpre[HPN][KSPLIT];
#pragma unroll
  for (int u = 0; u < HPN; ++u) {
    const int e = tid + u * kSplitThreads, row = e / HP, n = e - row * HP;
#pragma unroll
    for (int qq = 0; qq < KSPLIT; ++qq)
      hpre[u][qq] = S.h1part[((int64_t)(slice * KSPLIT + qq) * ROWS + row) * HP + n];
  }
  const int q4 = qw >> 2;
  constexpr int XG = (ROWS * (XQ / 4) + kSplitThreads - 1) / kSplitThreads;     // 4
  float4 xg[XG];
  {
    const float* __restrict__ xq = S.xq + ((int64_t)(slice * KSPLIT + q) * ROWS) * XQ;
#pragma unroll
    for (int u = 0; u < XG; ++u) {
      const int e = tid + u * kSplitThreads;
      xg[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < ROWS * q4) {
        const int rr = e / q4, c = e - rr * q4;
        xg[u] = *reinterpret_cast<const float4*>(xq + rr * XQ + 4 * c);
      }
    }
  }
  constexpr int W2N = (HP * HS + kSplitThreads - 1) / kSplitThreads;            // 17
  float w2r[W2N];
#pragma unroll
  for (int u = 0; u < W2N; ++u) {
    const int e = tid + u * kSplitThreads, m = e / HS, k = e - m * HS;
    w2r[u] = (e < HP * HS && m < H2 && k < H1) ? P.W2[m * H1 + k] : 0.f;
  }
  constexpr int W3N = (OP * HS + kSplitThreads - 1) / kSplitThreads;            // 5
  float w3r[W3N];
#pragma unroll
  for (int u = 0; u < W3N; ++u) {
    const int e = tid + u * kSplitThreads, m = e / HS, k = e - m * HS;
    w3r[u] = (e < OP * HS && m < OUT && k < H2) ? P.W3[m * H2 + k] : 0.f;
  }
  if (tid < HP) {
    bs[tid] = tid < H1 ? P.b1[tid] : 0.f;
    bs[HP + tid] = tid < H2 ? P.b2[tid] : 0.f;
    bs[2 * HP + tid] = tid < OUT ? P.b3[tid] : 0.f;
  }
  if (tid < ROWS) ys[tid] = S.ys[slice * ROWS + tid];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < HPN; ++u) {
    const int e = tid + u * kSplitThreads, row = e / HP, n = e - row * HP;
    mlp_combine1(lds, H1, row, n, hpre[u][0], hpre[u][1], hpre[u][2], hpre[u][3]);
  }
#pragma unroll
  for (int u = 0; u < W2N; ++u) {
    const int e = tid + u * kSplitThreads;
    if (e < HP * HS) w2s[e] = w2r[u];
  }
#pragma unroll
  for (int u = 0; u < W3N; ++u) {
    const int e = tid + u * kSplitThreads;
    if (e < OP * HS) w3s[e] = w3r[u];
  }
#pragma unroll
  for (int u = 0; u < XG; ++u) {
    const int e = tid + u * kSplitThreads;
    if (e < ROWS * q4) {
      const int rr = e / q4, c = e - rr * q4;
      *reinterpret_cast<float4*>(xs + rr * XQS + 4 * c) = xg[u];
    }
  }
  __syncthreads();
  // ---- the middle, in every workgroup of the slice: wave = column tile
  mlp_forward2(lds, H2, wave, r, g);
  __syncthreads();
  if (wave == 0) mlp_forward3(lds, r, g);
  __syncthreads();
  mlp_softmax_ce(lds, OUT, P.inv_softmax_temp, invB, tid);  // (256 threads = 16 x 16 logits)
  __syncthreads();
  if (lead && tid == 0) mlp_loss_sums(lds, P.loss_part + slice, P.correct_part + slice);
  if (lead) {
    mlp_dW3_tile(lds, gp + P.off_W3, OUT, H2, wave, r, g);
    if (tid < OUT) gp[P.off_b3 + tid] = mlp_column_sum(dfs, OP, tid);
  }
  mlp_backward3_d2(lds, wave, r, g);
  __syncthreads();
  if (lead) {  // dW2: wave = row tile, all four column tiles
    float a[ROWS / 4];
    mlp_dT_fragment(a, d2s, 16 * wave, r, g);
#pragma unroll
    for (int t = 0; t < HP / 16; ++t) mlp_dW2_tile(lds, a, gp + P.off_W2, H1, H2, 16 * wave, t, r, g);
    if (tid < H2) gp[P.off_b2 + tid] = mlp_column_sum(d2s, HS, tid);
  }
  mlp_backward2_d1(lds, wave, r, g);
  __syncthreads();
  if (lead && tid < H1) gp[P.off_b1 + tid] = mlp_column_sum(d1s, HS, tid);
  {  // backward 1: this workgroup's quarter of the input columns, two tiles at a time; wave = hidden-unit tile
    float a[ROWS / 4];
    mlp_dT_fragment(a, d1s, 16 * wave, r, g);
    const int tiles = j1 - j0;
    for (int t = 0; t < tiles; t += 2)
      mlp_dW1_pair(lds, a, xs, XQS, t, t + 1, t + 1 < tiles, c0, gp + P.off_W1, H1, IN, 16 * wave, lane);
  }
}

__global__ __launch_bounds__(kSplitThreads) void mlp_rest_kernel(sgmcmc_mlp_args P, sgmcmc_layout L,
                                                                 sgmcmc_step_args Aprev, int with_finalize) {
  mlp_rest_body(P, L, Aprev, with_finalize);
}

// ---- several independent chains per launch (blockIdx.y = chain): the small nets use 33-46 workgroups of a
// 256-CU GPU per launch; K chains of the same architecture stepped in lock-step share the three launches of a
// leapfrog step.  Per-chain pointers (weights, partial-gradient scratch, sampler arena) come from a device-resident
// table written once; what changes per step -- the transition's scalars (one block when every chain has the same
// schedule, else one block per chain: the *_args kernels below) and each chain's 128 row indices -- travels BY VALUE
// in the kernel arguments (16-bit indices: 8 chains x 256 B).
struct IdxMulti { uint16_t idx[SGMCMC_MAX_CHAINS][SGMCMC_MLP_BATCH_MULTI]; };

__global__ __launch_bounds__(kSplitThreads) void mlp_f1_multi_kernel(const sgmcmc_dense_chain* __restrict__ T,
                                                                     IdxMulti IM) {
  const int c = blockIdx.y;
  const sgmcmc_mlp_args P = T[c].mlp;
  mlp_f1_body(P, nullptr, IM.idx[c]);
}

// chain blockIdx.y of the table with ITS block of transition scalars (the deferred finalize's), wherever that came from
__device__ __forceinline__ void mlp_rest_chain(const sgmcmc_dense_chain* __restrict__ T, sgmcmc_step_args Aprev,
                                               int with_finalize) {
  const int c = blockIdx.y;
  const sgmcmc_mlp_args P = T[c].mlp;
  const sgmcmc_layout L = T[c].layout;
  Aprev.stream = T[c].chain_id;
  mlp_rest_body(P, L, Aprev, with_finalize);
}

__global__ __launch_bounds__(kSplitThreads) void mlp_rest_multi_kernel(const sgmcmc_dense_chain* __restrict__ T,
                                                                       sgmcmc_step_args Aprev, int with_finalize) {
  mlp_rest_chain(T, Aprev, with_finalize);
}

extern "C++" {
template <int KIND>
__device__ __forceinline__ void step_parts_chain(const sgmcmc_dense_chain* __restrict__ T, sgmcmc_step_args A) {
  const int c = blockIdx.y;
  const sgmcmc_layout L = T[c].layout;
  const sgmcmc_mlp_args& M = T[c].mlp;
  const int slices = (M.batch + ROWS - 1) / ROWS;
  const GradParts G = {M.gpart, slices, M.gpart_stride, M.loss_part, M.correct_part, M.batch, T[c].num_data};
  A.stream = T[c].chain_id;
  const Early<float, 1> E = step_early<float, true, 1>(L, A.chunk_begin);
  step_body<float, KIND, true, 1, true, false, false, true>(L, A, G, &E);
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void step_parts_multi_kernel(const sgmcmc_dense_chain* __restrict__ T,
                                                                    sgmcmc_step_args A) {
  step_parts_chain<KIND>(T, A);
}

// ---- the same launches with EACH chain's own transition scalars (a temperature ladder, a step-size sweep): chain c
// reads block c of an array passed by value (8 x 128 B = 1 KiB of kernel arguments; the 2 KiB of row indices go to the
// other launch).  blockIdx.y is a workgroup id, so the block is wave-uniform and lands in SGPRs as the single block
// does; every decision of the transition body (draw / no draw, momentum decay, clamp) is taken from it.
struct ArgsMulti { sgmcmc_step_args a[SGMCMC_MAX_CHAINS]; };

template <int KIND>
__global__ __launch_bounds__(kThreads) void step_parts_multi_args_kernel(const sgmcmc_dense_chain* __restrict__ T,
                                                                         ArgsMulti AM) {
  step_parts_chain<KIND>(T, AM.a[blockIdx.y]);
}
}  // extern "C++"

__global__ __launch_bounds__(kSplitThreads) void mlp_rest_multi_args_kernel(const sgmcmc_dense_chain* __restrict__ T,
                                                                            ArgsMulti AM, int with_finalize) {
  mlp_rest_chain(T, AM.a[blockIdx.y], with_finalize);
}
}  // namespace

int64_t sgmcmc_mlp_split_scratch_floats(int batch) {
  const int64_t slices = (batch + ROWS - 1) / ROWS;
  return slices * ((int64_t)KSPLIT * ROWS * HP + (int64_t)KSPLIT * ROWS * XQ + ROWS);
}

__attribute__((visibility("hidden"))) int sgmcmc_step_parts_value(const sgmcmc_layout* L, const sgmcmc_step_args* A,
                                                                  const sgmcmc_grad_parts* P, void* stream);  // sgmcmc_hip.hip

int sgmcmc_dense_step_direct(const sgmcmc_layout* L, const sgmcmc_mlp_args* mlp,
                             const sgmcmc_step_args* A, double num_data, const int64_t* idx_host,
                             const sgmcmc_step_args* A_pending, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!L || !mlp || !A || !idx_host || mlp->batch > SGMCMC_MLP_MAX_INLINE || !dense_shape_ok(*mlp))
    return (int)hipErrorInvalidValue;
  if (A_pending && !(A_pending->flags & SGMCMC_SMALL_FINALIZE)) return (int)hipErrorInvalidValue;
  const int64_t lds = sgmcmc_mlp_lds_bytes(mlp->in_features);
  static int64_t granted = 0;
  const hipError_t e = grant_dynamic_lds({reinterpret_cast<const void*>(mlp_fwdbwd_kernel_inline),
                                          reinterpret_cast<const void*>(mlp_fwdbwd_kernel_inline_fin)}, lds, granted);
  if (e != hipSuccess) return (int)e;
  IdxBlock IB;
  for (int b = 0; b < mlp->batch; ++b) IB.idx[b] = (int32_t)idx_host[b];
  const int slices = (mlp->batch + ROWS - 1) / ROWS;
  hipStream_t s = (hipStream_t)stream;
  if (mlp->split_scratch && dense_shape_ok(*mlp, true)) {
    sgmcmc_step_args Ap = A_pending ? *A_pending : *A;
    Ap.flags &= ~(uint32_t)SGMCMC_DEFER_FINALIZE;
    SGMCMC_LAUNCH(mlp_f1_kernel, dim3((unsigned)(slices * KSPLIT)), dim3(kSplitThreads), 0, s, *mlp, IB);
    SGMCMC_LAUNCH(mlp_rest_kernel, dim3((unsigned)(slices * KSPLIT + (A_pending ? 1 : 0))),
                       dim3(kSplitThreads), 0, s, *mlp, *L, Ap, A_pending ? 1 : 0);
  } else if (A_pending) {
    sgmcmc_step_args Ap = *A_pending;
    Ap.flags &= ~(uint32_t)SGMCMC_DEFER_FINALIZE;
    SGMCMC_LAUNCH(mlp_fwdbwd_kernel_inline_fin, dim3((unsigned)slices + 1), dim3(kMlpThreads),
                       (size_t)lds, s, *mlp, IB, *L, Ap);
  } else {
    SGMCMC_LAUNCH(mlp_fwdbwd_kernel_inline, dim3((unsigned)slices), dim3(kMlpThreads), (size_t)lds, s,
                       *mlp, IB);
  }
  const sgmcmc_grad_parts G = grad_parts_of(*mlp, num_data);
  return sgmcmc_step_parts_value(L, A, &G, s);
}

namespace {
// what both multi-chain entry points require of chain 0's record and of the (first) block
bool dense_multi_ok(const sgmcmc_dense_chain* chains_dev, const sgmcmc_dense_chain* chain0_host, int n_chains,
                    const sgmcmc_step_args* A, const uint16_t* idx_host) {
  if (!chains_dev || !chain0_host || !A || !idx_host || n_chains <= 0 || n_chains > SGMCMC_MAX_CHAINS) return false;
  const sgmcmc_mlp_args& mlp = chain0_host->mlp;
  const sgmcmc_layout& L = chain0_host->layout;
  return mlp.batch <= SGMCMC_MLP_BATCH_MULTI && mlp.split_scratch && dense_shape_ok(mlp, true) &&
         L.dtype == SGMCMC_F32 && L.chunk_elems == SGMCMC_CHUNK_SMALL && !(A->flags & SGMCMC_UNALIGNED) &&
         (A->flags & SGMCMC_SMALL_FINALIZE) && (A->flags & SGMCMC_DEFER_FINALIZE);
}

void fill_idx_multi(IdxMulti& IM, const uint16_t* idx_host, int n_chains, int batch) {
  for (int c = 0; c < n_chains; ++c)
    for (int b = 0; b < batch; ++b) IM.idx[c][b] = idx_host[(size_t)c * batch + b];
}

// the three launches of a lock-step step, after the entry point's validation.  A / A_pending: ONE block for all chains
// (the 128-byte kernel argument), or with `per_chain` n_chains blocks each
int dense_step_multi_launch(const sgmcmc_dense_chain* chains_dev, const sgmcmc_mlp_args& mlp, int n_chains,
                            const sgmcmc_step_args* A, const uint16_t* idx_host, const sgmcmc_step_args* A_pending,
                            bool per_chain, hipStream_t s) {
  if (A->kind != SGMCMC_VERLET && A->kind != SGMCMC_HMC && A->kind != SGMCMC_SGLD) return (int)hipErrorInvalidValue;
  IdxMulti IM;
  fill_idx_multi(IM, idx_host, n_chains, mlp.batch);
  ArgsMulti AM, AP;  // [0] alone when one block serves all chains (unused rows repeat chain 0: no uninitialised kernel argument)
  for (int c = 0; c < SGMCMC_MAX_CHAINS; ++c) {
    const int k = per_chain && c < n_chains ? c : 0;
    AM.a[c] = A[k];
    AP.a[c] = A_pending ? A_pending[k] : A[k];
    AP.a[c].flags &= ~(uint32_t)SGMCMC_DEFER_FINALIZE;
  }
  const int slices = (mlp.batch + ROWS - 1) / ROWS, fin = A_pending ? 1 : 0;
  const unsigned ny = (unsigned)n_chains;
  const dim3 split(kSplitThreads), rest_grid((unsigned)(slices * KSPLIT + fin), ny);
  SGMCMC_LAUNCH(mlp_f1_multi_kernel, dim3((unsigned)(slices * KSPLIT), ny), split, 0, s, chains_dev, IM);
  if (per_chain)
    SGMCMC_LAUNCH(mlp_rest_multi_args_kernel, rest_grid, split, 0, s, chains_dev, AP, fin);
  else
    SGMCMC_LAUNCH(mlp_rest_multi_kernel, rest_grid, split, 0, s, chains_dev, AP.a[0], fin);
  const dim3 grid((unsigned)(A->chunk_end - A->chunk_begin), ny), block(kThreads);
#define STEP_PARTS_MULTI(KIND)                                                                         \
  if (per_chain)                                                                                       \
    SGMCMC_LAUNCH(step_parts_multi_args_kernel<KIND>, grid, block, 0, s, chains_dev, AM);              \
  else                                                                                                 \
    SGMCMC_LAUNCH(step_parts_multi_kernel<KIND>, grid, block, 0, s, chains_dev, AM.a[0])
  switch (A->kind) {
    case SGMCMC_VERLET: STEP_PARTS_MULTI(SGMCMC_VERLET); break;
    case SGMCMC_HMC: STEP_PARTS_MULTI(SGMCMC_HMC); break;
    default: STEP_PARTS_MULTI(SGMCMC_SGLD); break;
  }
#undef STEP_PARTS_MULTI
  return (int)hipGetLastError();
}
}  // namespace

int sgmcmc_dense_step_multi(const sgmcmc_dense_chain* chains_dev, const sgmcmc_dense_chain* chain0_host, int n_chains,
                            const sgmcmc_step_args* A, const uint16_t* idx_host, const sgmcmc_step_args* A_pending,
                            void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!dense_multi_ok(chains_dev, chain0_host, n_chains, A, idx_host)) return (int)hipErrorInvalidValue;
  return dense_step_multi_launch(chains_dev, chain0_host->mlp, n_chains, A, idx_host, A_pending, false,
                                 (hipStream_t)stream);
}

int sgmcmc_dense_step_multi_args(const sgmcmc_dense_chain* chains_dev, const sgmcmc_dense_chain* chain0_host,
                                 int n_chains, const sgmcmc_step_args* A, const uint16_t* idx_host,
                                 const sgmcmc_step_args* A_pending, void* stream) {
  // host-side validation first: nothing below touches the runtime before the blocks are known to agree
  if (!dense_multi_ok(chains_dev, chain0_host, n_chains, A, idx_host)) return (int)hipErrorInvalidValue;
  if (A->kind != SGMCMC_VERLET && A->kind != SGMCMC_HMC && A->kind != SGMCMC_SGLD) return (int)hipErrorInvalidValue;
  if (A->chunk_end <= A->chunk_begin) return (int)hipErrorInvalidValue;
  // the template parameter, the launch geometry, the sweep counter and the metric cadence are one per launch
  for (const sgmcmc_step_args* B : {A, A_pending}) {
    if (!B) continue;
    for (int c = 1; c < n_chains; ++c)
      if (B[c].kind != B[0].kind || B[c].flags != B[0].flags || B[c].seg_begin != B[0].seg_begin ||
          B[c].seg_end != B[0].seg_end || B[c].chunk_begin != B[0].chunk_begin || B[c].chunk_end != B[0].chunk_end ||
          B[c].draw != B[0].draw)
        return (int)hipErrorInvalidValue;
  }
  if (A_pending && !(A_pending->flags & SGMCMC_SMALL_FINALIZE)) return (int)hipErrorInvalidValue;
  SGMCMC_FRESH_ERROR_STATE();
  return dense_step_multi_launch(chains_dev, chain0_host->mlp, n_chains, A, idx_host, A_pending, true,
                                 (hipStream_t)stream);
}

namespace {
__global__ __launch_bounds__(256) void accumulate_parts_kernel(const float* __restrict__ gpart,
                                                               int n_slices, int64_t stride,
                                                               double* __restrict__ acc,
                                                               float* __restrict__ out, int64_t n,
                                                               const float* __restrict__ loss_part,
                                                               const float* __restrict__ correct_part,
                                                               double* __restrict__ stats, int first) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) {
    double a = first ? 0.0 : acc[j];
    for (int s = 0; s < n_slices; ++s) a += (double)gpart[(int64_t)s * stride + j];
    acc[j] = a;
    if (out) out[j] = (float)a;
  }
  if (stats && j == 0) {
    double l = first ? 0.0 : stats[0], c = first ? 0.0 : stats[1];
    for (int s = 0; s < n_slices; ++s) { l += (double)loss_part[s]; c += (double)correct_part[s]; }
    stats[0] = l; stats[1] = c;
  }
}
}  // namespace

int sgmcmc_accumulate_parts(const float* gpart, int n_slices, int64_t stride, double* acc,
                            float* out_f32, int64_t n, const float* loss_part,
                            const float* correct_part, double* stats, int first, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!gpart || !acc || n_slices <= 0 || n <= 0 || n > stride) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(accumulate_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, gpart, n_slices, stride, acc, out_f32, n, loss_part,
                     correct_part, stats, first);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- native stepper
struct sgmcmc_dense_stepper {
  hipGraph_t* graphs = nullptr;       // one replica per pinned slot (its host address is baked in)
  hipGraphExec_t* execs = nullptr;
  hipStream_t capture_stream = nullptr;
  hipEvent_t* events = nullptr;
  unsigned char* used = nullptr;
  unsigned char* pinned = nullptr;
  int n_ring = 0, batch = 0;
  int64_t slot_bytes = 0;
  uint64_t k = 0;
};

int sgmcmc_dense_stepper_create(const sgmcmc_layout* L, const sgmcmc_mlp_args* mlp,
                                const sgmcmc_step_args* A_geometry, double num_data,
                                void* dev_args, void* pinned, int n_ring, int64_t slot_bytes,
                                sgmcmc_dense_stepper** out) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!L || !mlp || !A_geometry || !dev_args || !pinned || n_ring <= 0 || !out ||
      slot_bytes < (int64_t)sizeof(sgmcmc_step_args) + 8 * (int64_t)mlp->batch || (slot_bytes & 7))
    return (int)hipErrorInvalidValue;
  sgmcmc_dense_stepper* S = new sgmcmc_dense_stepper();
  S->n_ring = n_ring; S->batch = mlp->batch; S->slot_bytes = slot_bytes;
  S->pinned = (unsigned char*)pinned;
  S->events = new hipEvent_t[n_ring];
  S->graphs = new hipGraph_t[n_ring]();
  S->execs = new hipGraphExec_t[n_ring]();
  S->used = new unsigned char[n_ring]();
  hipError_t err = hipStreamCreateWithFlags(&S->capture_stream, hipStreamNonBlocking);
  for (int i = 0; i < n_ring && err == hipSuccess; ++i)
    err = hipEventCreateWithFlags(&S->events[i], hipEventDisableTiming);
  if (err != hipSuccess) return (int)err;
  const sgmcmc_grad_parts G = grad_parts_of(*mlp, num_data);
  // one eager pass first: loads the code objects and sets the LDS attribute outside capture
  // (writes scratch only: idx = identity, no argument forwarding)
  sgmcmc_mlp_args warm = *mlp;
  warm.idx = nullptr; warm.args_src = nullptr; warm.args_dst = nullptr; warm.args_bytes = 0;
  int rc = sgmcmc_mlp_fwdbwd(&warm, S->capture_stream);
  if (rc) return rc;
  err = hipStreamSynchronize(S->capture_stream);
  if (err != hipSuccess) return (int)err;
  for (int i = 0; i < n_ring; ++i) {
    unsigned char* slot = S->pinned + (int64_t)i * slot_bytes;
    sgmcmc_mlp_args m = *mlp;
    m.args_src = slot;
    m.args_dst = dev_args;
    m.args_bytes = (int32_t)sizeof(sgmcmc_step_args);
    m.idx = reinterpret_cast<const int64_t*>(slot + sizeof(sgmcmc_step_args));
    err = hipStreamBeginCapture(S->capture_stream, hipStreamCaptureModeThreadLocal);
    if (err != hipSuccess) return (int)err;
    rc = sgmcmc_mlp_fwdbwd(&m, S->capture_stream);
    if (!rc)
      rc = sgmcmc_step_indirect_parts(L, A_geometry, (const sgmcmc_step_args*)dev_args, &G,
                                      S->capture_stream);
    err = hipStreamEndCapture(S->capture_stream, &S->graphs[i]);
    if (rc) return rc;
    if (err != hipSuccess) return (int)err;
    err = hipGraphInstantiate(&S->execs[i], S->graphs[i], nullptr, nullptr, 0);
    if (err != hipSuccess) return (int)err;
  }
  *out = S;
  return 0;
}

int sgmcmc_dense_stepper_step(sgmcmc_dense_stepper* S, const sgmcmc_step_args* A,
                              const int64_t* idx_host, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!S || !A || !idx_host) return (int)hipErrorInvalidValue;
  const int i = (int)(S->k % (uint64_t)S->n_ring);
  ++S->k;
  hipError_t err;
  if (S->used[i]) {  // the replay that last read this slot must have finished
    err = hipEventSynchronize(S->events[i]);
    if (err != hipSuccess) return (int)err;
  }
  unsigned char* slot = S->pinned + (int64_t)i * S->slot_bytes;
  memcpy(slot, A, sizeof(sgmcmc_step_args));
  memcpy(slot + sizeof(sgmcmc_step_args), idx_host, 8 * (size_t)S->batch);
  hipStream_t s = (hipStream_t)stream;
  err = hipGraphLaunch(S->execs[i], s);
  if (err != hipSuccess) return (int)err;
  S->used[i] = 1;
  return (int)hipEventRecord(S->events[i], s);
}

int sgmcmc_dense_stepper_destroy(sgmcmc_dense_stepper* S) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!S) return 0;
  for (int i = 0; i < S->n_ring; ++i) {
    if (S->execs && S->execs[i]) (void)hipGraphExecDestroy(S->execs[i]);
    if (S->graphs && S->graphs[i]) (void)hipGraphDestroy(S->graphs[i]);
    (void)hipEventDestroy(S->events[i]);
  }
  if (S->capture_stream) (void)hipStreamDestroy(S->capture_stream);
  delete[] S->events;
  delete[] S->graphs;
  delete[] S->execs;
  delete[] S->used;
  delete S;
  return 0;
}

}  // extern "C"
