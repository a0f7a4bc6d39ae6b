// y = maxpool2x2( relu( x + bias_c ) ) of the convolutional classifier (models/conv_nets.py:44-56:
// Conv2d(+bias) -> ReLU -> MaxPool2d(2)), forward and backward, NCHW fp32, H and W even.
//
//   forward   y[n,c,i,j] = max(0, max_{di,dj} x[n,c,2i+di,2j+dj] + b[c])
//   backward  the gradient of y[n,c,i,j] goes to the FIRST maximal element of its window in scan order
//             (as ATen's max_pool2d) if that element's pre-activation is positive, nowhere otherwise;
//             dx is written in full (zeros included: no separate fill); dbias[c] = sum of the routed
//             gradients, as per-block partials [slice][channel] summed in a fixed order by the caller
//             (sgmcmc_wrw_reduce_many) -- no atomics.
//
// One thread per output element; block = (channel, slice of the batch) so that the bias and its gradient
// partial are per-block scalars.  HBM-bound: forward reads x, writes y/4; backward reads x and dy, writes dx.

namespace pool {

constexpr int kT = 256;

struct Geo {
  int N, C, H, W, S, NB;  // images, channels, input height/width, slices, images per slice
};

inline bool geo(int N, int C, int H, int W, Geo* g) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return false;
  int S = 512 / C;
  if (S < 1) S = 1;
  if (S > N) S = N;
  g->N = N; g->C = C; g->H = H; g->W = W;
  g->NB = (N + S - 1) / S;
  g->S = (N + g->NB - 1) / g->NB;
  return true;
}

__global__ __launch_bounds__(kT) void fwd_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                 float* __restrict__ y, Geo g) {
  const int c = blockIdx.x % g.C, s = blockIdx.x / g.C;
  const int n0 = s * g.NB, n1 = min(g.N, n0 + g.NB);
  const int HO = g.H >> 1, WO = g.W >> 1, PO = HO * WO;
  const float b = bias ? bias[c] : 0.f;
  for (int i = threadIdx.x; i < (n1 - n0) * PO; i += kT) {
    const int n = n0 + i / PO, p = i % PO, oi = p / WO, oj = p % WO;
    const float* __restrict__ src = x + (((size_t)n * g.C + c) * g.H + 2 * oi) * g.W + 2 * oj;
    const float2 r0 = *reinterpret_cast<const float2*>(src);
    const float2 r1 = *reinterpret_cast<const float2*>(src + g.W);
    int code;
    y[((size_t)n * g.C + c) * PO + p] = conv::pool_window(r0, r1, b, &code);
  }
}

__global__ __launch_bounds__(kT) void bwd_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                 const float* __restrict__ dy, float* __restrict__ dx,
                                                 float* __restrict__ dbias_part, Geo g) {
  const int c = blockIdx.x % g.C, s = blockIdx.x / g.C;
  const int n0 = s * g.NB, n1 = min(g.N, n0 + g.NB);
  const int HO = g.H >> 1, WO = g.W >> 1, PO = HO * WO;
  const float b = bias ? bias[c] : 0.f;
  float acc = 0.f;
  for (int i = threadIdx.x; i < (n1 - n0) * PO; i += kT) {
    const int n = n0 + i / PO, p = i % PO, oi = p / WO, oj = p % WO;
    const size_t off = (((size_t)n * g.C + c) * g.H + 2 * oi) * g.W + 2 * oj;
    const float2 r0 = *reinterpret_cast<const float2*>(x + off);
    const float2 r1 = *reinterpret_cast<const float2*>(x + off + g.W);
    int code;      // (recomputed from x: this operator keeps no byte)
    conv::pool_window(r0, r1, b, &code);
    acc += conv::unpool_window(dx + off, g.W, dy[((size_t)n * g.C + c) * PO + p], code);
  }
  if (dbias_part) {
    __shared__ float sh[kT / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) dbias_part[(size_t)s * g.C + c] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  }
}

}  // namespace pool

extern "C" int sgmcmc_pool_slices(int n, int channels, int h, int w) {
  pool::Geo g;
  return pool::geo(n, channels, h, w, &g) ? g.S : -1;
}

extern "C" int sgmcmc_bias_relu_pool_fwd(const float* x, const float* bias, float* y, int n, int channels,
                                         int h, int w, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  pool::Geo g;
  if (!x || !y || !pool::geo(n, channels, h, w, &g)) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(pool::fwd_kernel, dim3((unsigned)(g.C * g.S)), dim3(pool::kT), 0, (hipStream_t)stream, x, bias,
                     y, g);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_bias_relu_pool_bwd(const float* x, const float* bias, const float* dy, float* dx,
                                         float* dbias_part, int n, int channels, int h, int w, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  pool::Geo g;
  if (!x || !dy || !dx || !pool::geo(n, channels, h, w, &g)) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(pool::bwd_kernel, dim3((unsigned)(g.C * g.S)), dim3(pool::kT), 0, (hipStream_t)stream, x, bias,
                     dy, dx, dbias_part, g);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// ONE row of the softmax cross-entropy, written once for its three callers: xent::fwd_kernel (a thread per row),
// head::loss_kernel and lin::fwd_loss_kernel (thread 0 of the row's workgroup).  Same operations in the same order
// for all of them, so the three routes give the same bits:
//   m = max_k x_k;  e_k = expf(x_k - m);  s = e_0 + e_1 + ... (in order);  p_k = e_k * (1 / s);
//   loss = logf(s) - (x_t - m)
// in : v[0 .. K) the row's logits (K <= KB; the loops have KB steps guarded by k < K, so KB == K folds the guard)
// out: v[k] = GRAD ? gscale * (p_k - [k == label]) : p_k;  returns the row's loss.
// The label rule (include/sgmcmc_hip.h, "Labels"): the int64 label is compared as 64 bits against [0, K); a label
// outside gives a NaN loss and no one-hot term (d = gscale * p), and no address is ever formed from a label -- x_t is
// selected by comparison, not read at an index.
namespace xent {

constexpr int kMaxK = 16;

template <int KB, bool GRAD>
__device__ __forceinline__ float row(float (&v)[KB], int K, int64_t label, float gscale) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (k < K) m = fmaxf(m, v[k]);
  float xt = 0.f, s = 0.f;
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (k < K) {
      if ((int64_t)k == label) xt = v[k];
      v[k] = expf(v[k] - m);
      s += v[k];
    }
  const float inv = 1.f / s;
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (k < K) v[k] = GRAD ? gscale * (v[k] * inv - ((int64_t)k == label ? 1.f : 0.f)) : v[k] * inv;
  // -log p_t = log s - (x_t - m)
  return (uint64_t)label < (uint64_t)K ? logf(s) - (xt - m) : __builtin_nanf("");
}

}  // namespace xent

// ------------------------------------------------------------------------------------------------
// The classifier head of the ResNet (google_resnet.py:103-110): global average pool over the whole
// feature map -> Flatten -> Linear, as one operator each way.
//   forward   pooled[n,c] = mean_p h[n,c,p];  logits[n,k] = b[k] + sum_c W[k,c] pooled[n,c]
//   backward  dpooled[n,c] = sum_k dlogits[n,k] W[k,c];  dh[n,c,p] = dpooled[n,c] / P
//             dW / db as per-row slabs  dlogits[n,k] * pooled[n,c]  /  dlogits[n,k]  (fixed-order reduction
//             with the convolutions' slabs: sgmcmc_wrw_reduce_many)
// One workgroup per row; C <= 64 channels, P a multiple of 16 with C * 4 <= 256 threads, K <= 16 classes.
namespace head {

constexpr int kT = 256, kMaxC = 64, kMaxK = xent::kMaxK;

__global__ __launch_bounds__(kT) void fwd_kernel(const float* __restrict__ h, const float* __restrict__ W,
                                                 const float* __restrict__ b, float* __restrict__ pooled,
                                                 float* __restrict__ logits, int C, int P, int K) {
  __shared__ float ps[kMaxC];
  const int n = blockIdx.x, t = threadIdx.x, c = t >> 2, q = t & 3;
  float s = 0.f;
  if (c < C) {
    const float* __restrict__ src = h + ((size_t)n * C + c) * P + q * (P / 4);
    for (int i = 0; i < P / 4; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(src + i);
      s += (v.x + v.y) + (v.z + v.w);
    }
  }
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  if (c < C && q == 0) {
    const float m = s / (float)P;
    ps[c] = m;
    pooled[(size_t)n * C + c] = m;
  }
  __syncthreads();
  if (t < K) {
    float a = b ? b[t] : 0.f;
    for (int j = 0; j < C; ++j) a += W[t * C + j] * ps[j];
    logits[(size_t)n * K + t] = a;
  }
}

// SUMS (P == 64, i.e. 16 float4 per channel plane): dh is the incoming gradient of the BatchNorm + ReLU that produced
// h; its backward sums over this image -- sum dz and sum dz * xhat, dz = dh * [h > 0] -- leave with the launch
// (partial[(c * N + n) * 2 + {0,1}]: a slice per image), as the convolution gradients' SUMS epilogue does.
struct HeadSums {
  const float* y;        // the BatchNorm's input
  const float* out;      // h itself (the ReLU mask)
  const float* mean;
  const float* invstd;
  double* partial;
  int group_rows;        // > 0: groups of this many rows, mean / invstd are [group][C] (bn_hip.inc, GROUPS)
};

template <bool SUMS>
__global__ __launch_bounds__(kT) void bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ pooled,
                                                 const float* __restrict__ W, float* __restrict__ dh,
                                                 float* __restrict__ slab_w, float* __restrict__ slab_b, int C,
                                                 int P, int K, HeadSums S) {
  __shared__ float dl[kMaxK], dp[kMaxC], pl[kMaxC];
  const int n = blockIdx.x, t = threadIdx.x;
  if (t < K) dl[t] = dlogits[(size_t)n * K + t];
  if (t < C) pl[t] = pooled[(size_t)n * C + t];
  __syncthreads();
  if (t < C) {
    float a = 0.f;
    for (int k = 0; k < K; ++k) a += dl[k] * W[k * C + t];
    dp[t] = a / (float)P;
  }
  __syncthreads();
  float* __restrict__ dst = dh + (size_t)n * C * P;
  const int go = (SUMS && S.group_rows > 0) ? (n / S.group_rows) * C : 0;      // (once per workgroup, not per element)
  for (int i = t; i < C * P / 4; i += kT) {
    const int c = (4 * i) / P;
    const float v = dp[c];
    sgmcmc_store4<8>(dh, dst + 4 * i, v, v, v, v);
    if (SUMS) {      // 16 consecutive lanes hold one channel's plane: fixed xor tree, lane 0 of the group writes
      const size_t off = (size_t)n * C * P + 4 * (size_t)i;
      const float4 o = *reinterpret_cast<const float4*>(S.out + off), q = *reinterpret_cast<const float4*>(S.y + off);
      const float m = S.mean[go + c], is = S.invstd[go + c];
      const float d0 = o.x > 0.f ? v : 0.f, d1 = o.y > 0.f ? v : 0.f, d2 = o.z > 0.f ? v : 0.f, d3 = o.w > 0.f ? v : 0.f;
      float z1 = (d0 + d1) + (d2 + d3);
      float z2 = (d0 * ((q.x - m) * is) + d1 * ((q.y - m) * is)) + (d2 * ((q.z - m) * is) + d3 * ((q.w - m) * is));
#pragma unroll
      for (int off2 = 1; off2 < 16; off2 <<= 1) { z1 += __shfl_xor(z1, off2, 64); z2 += __shfl_xor(z2, off2, 64); }
      if ((t & 15) == 0) {
        S.partial[((size_t)c * gridDim.x + n) * 2] = (double)z1;
        S.partial[((size_t)c * gridDim.x + n) * 2 + 1] = (double)z2;
      }
    }
  }
  if (slab_w)
    for (int i = t; i < K * C; i += kT) slab_w[(size_t)n * K * C + i] = dl[i / C] * pl[i % C];
  if (slab_b && t < K) slab_b[(size_t)n * K + t] = dl[t];
}

// Round 3: the classifier head, the softmax cross-entropy on its logits and BOTH backward passes in ONE launch.
// Everything between the trunk's last activation h and its gradient dh is per image: pooled -> logits ->
// d loss / d logits (xent::fwd_kernel<GRAD>'s arithmetic, thread 0 of the row) -> dpooled -> dh, the row's terms of
// dW / db, and (SUMS) the last BatchNorm's backward sums.  Replaces head::fwd_kernel + xent::fwd_kernel<true> +
// head::bwd_kernel of a gradient evaluation (three launches of ~5 us each, every one at the launch floor).
// loss_rows[n] = -log softmax(logits_n)[y_n] (unscaled); dlogits = gscale (p - onehot).
// counters (optional): block 0 adds 1 to n_counters int64 values -- the BatchNorm layers' num_batches_tracked, one
// contiguous array (models/nets.py): the ATen launch that did this is gone too.
template <bool SUMS>
__global__ __launch_bounds__(kT) void loss_kernel(const float* __restrict__ h, const float* __restrict__ W,
                                                  const float* __restrict__ b, const int64_t* __restrict__ y,
                                                  float* __restrict__ pooled, float* __restrict__ logits,
                                                  float* __restrict__ dlogits, float* __restrict__ loss_rows,
                                                  float* __restrict__ dh, float* __restrict__ slab_w,
                                                  float* __restrict__ slab_b, int C, int P, int K, float gscale,
                                                  HeadSums S, long long* __restrict__ counters, int n_counters) {
  __shared__ float ps[kMaxC], lg[kMaxK], dl[kMaxK], dp[kMaxC];
  __shared__ float Ws[kMaxK * kMaxC];      // the weights: read 2 (K + C) times per row below, from LDS instead of L2
  const int n = blockIdx.x, t = threadIdx.x, c = t >> 2, q = t & 3;
  // EVERY global operand of the row is requested here, before the first use: the launch is a chain of phases (pooling ->
  // logits -> loss -> dpooled -> dh) and each of these was a round trip of its own in the middle of it -- the counters
  // (block 0 began with load -> wait -> store), the bias, the label, and (SUMS) the mask / BatchNorm-input elements and
  // saved statistics of this thread's (up to kPre) float4 of dh
  const bool counting = counters && n == 0 && t < n_counters;
  // (an unconditional load from an address that is always valid: a value defined inside a branch is waited for at its end)
  const long long cnt = (counting ? counters : reinterpret_cast<const long long*>(y))[counting ? t : 0];
  const float bias_t = (b && t < K) ? b[t] : 0.f;
  const int64_t tgt_pre = t == 0 ? y[n] : 0;
  constexpr int kPre = 4;
  float4 pre_o[kPre], pre_q[kPre];
  float pre_m[kPre], pre_is[kPre];
  const int go = (SUMS && S.group_rows > 0) ? (n / S.group_rows) * C : 0;      // (once per workgroup, not per element)
  if (SUMS) {
#pragma unroll
    for (int u = 0; u < kPre; ++u) {
      const int i = t + u * kT;
      if (i < C * P / 4) {
        const size_t off = (size_t)n * C * P + 4 * (size_t)i;
        pre_o[u] = *reinterpret_cast<const float4*>(S.out + off);
        pre_q[u] = *reinterpret_cast<const float4*>(S.y + off);
        pre_m[u] = S.mean[go + (4 * i) / P];
        pre_is[u] = S.invstd[go + (4 * i) / P];
      }
    }
  }
  // every global operand of the row's first phase is requested before the first use (a `for (...) Ws[i] = W[i]` loop
  // and the pooling loop compile to load -> wait -> use per iteration: 7 round trips in a row of a 10 us launch)
  constexpr int kWPer = (kMaxK * kMaxC + kT - 1) / kT;
  float wr[kWPer];
#pragma unroll
  for (int u = 0; u < kWPer; ++u) { const int i = t + u * kT; wr[u] = i < K * C ? W[i] : 0.f; }
  float s = 0.f;
  if (c < C) {
    const float* __restrict__ src = h + ((size_t)n * C + c) * P + q * (P / 4);
    if (P == 64) {        // (the trunk's 8 x 8 maps: 4 float4 per thread)
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float4*>(src + 4 * j);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    } else {
      for (int i = 0; i < P / 4; i += 4) {
        const float4 v = *reinterpret_cast<const float4*>(src + i);
        s += (v.x + v.y) + (v.z + v.w);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kWPer; ++u) { const int i = t + u * kT; if (i < K * C) Ws[i] = wr[u]; }
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  if (c < C && q == 0) {
    const float m = s / (float)P;
    ps[c] = m;
    pooled[(size_t)n * C + c] = m;
  }
  __syncthreads();
  if (t < K) {
    float a = bias_t;
    for (int j = 0; j < C; ++j) a += Ws[t * C + j] * ps[j];
    lg[t] = a;
    logits[(size_t)n * K + t] = a;
  }
  __syncthreads();
  if (t == 0) {       // the row's softmax cross-entropy (xent::row: a label outside [0, K), e.g. an ignore index, gives a
    float v[kMaxK];   // NaN loss row and never an out-of-bounds read of the logits)
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) v[k] = lg[k];
    loss_rows[n] = xent::row<kMaxK, true>(v, K, tgt_pre, gscale);
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) { dl[k] = v[k]; dlogits[(size_t)n * K + k] = v[k]; }
  }
  __syncthreads();
  if (t < C) {
    float a = 0.f;
    for (int k = 0; k < K; ++k) a += dl[k] * Ws[k * C + t];
    dp[t] = a / (float)P;
  }
  __syncthreads();
  float* __restrict__ dst = dh + (size_t)n * C * P;
#pragma unroll 4
  for (int i = t, u = 0; i < C * P / 4; i += kT, ++u) {
    const int cc = (4 * i) / P;
    const float v = dp[cc];
    sgmcmc_store4<8>(dh, dst + 4 * i, v, v, v, v);
    if (SUMS) {
      const size_t off = (size_t)n * C * P + 4 * (size_t)i;
      float4 o, qq;
      float m, is;
      if (u < kPre) { o = pre_o[u]; qq = pre_q[u]; m = pre_m[u]; is = pre_is[u]; }
      else {
        o = *reinterpret_cast<const float4*>(S.out + off); qq = *reinterpret_cast<const float4*>(S.y + off);
        m = S.mean[go + cc]; is = S.invstd[go + cc];
      }
      const float d0 = o.x > 0.f ? v : 0.f, d1 = o.y > 0.f ? v : 0.f, d2 = o.z > 0.f ? v : 0.f, d3 = o.w > 0.f ? v : 0.f;
      float z1 = (d0 + d1) + (d2 + d3);
      float z2 = (d0 * ((qq.x - m) * is) + d1 * ((qq.y - m) * is)) + (d2 * ((qq.z - m) * is) + d3 * ((qq.w - m) * is));
#pragma unroll
      for (int off2 = 1; off2 < 16; off2 <<= 1) { z1 += __shfl_xor(z1, off2, 64); z2 += __shfl_xor(z2, off2, 64); }
      if ((t & 15) == 0) {
        S.partial[((size_t)cc * gridDim.x + n) * 2] = (double)z1;
        S.partial[((size_t)cc * gridDim.x + n) * 2 + 1] = (double)z2;
      }
    }
  }
  if (slab_w)
    for (int i = t; i < K * C; i += kT) slab_w[(size_t)n * K * C + i] = dl[i / C] * ps[i % C];
  if (slab_b && t < K) slab_b[(size_t)n * K + t] = dl[t];
  if (counting) counters[t] = cnt + 1;
}

inline bool ok(int n, int C, int P, int K) {
  return n > 0 && C > 0 && C <= kMaxC && C * 4 <= kT && P > 0 && P % 16 == 0 && K > 0 && K <= kMaxK;
}

}  // namespace head

extern "C" int sgmcmc_pool_linear_fwd(const float* h, const float* weight, const float* bias, float* pooled,
                                      float* logits, int n, int channels, int plane, int classes, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!h || !weight || !pooled || !logits || !head::ok(n, channels, plane, classes)) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(head::fwd_kernel, dim3((unsigned)n), dim3(head::kT), 0, (hipStream_t)stream, h, weight, bias,
                     pooled, logits, channels, plane, classes);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_pool_linear_bwd(const float* dlogits, const float* pooled, const float* weight, float* dh,
                                      float* slab_w, float* slab_b, int n, int channels, int plane, int classes,
                                      void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!dlogits || !pooled || !weight || !dh || !head::ok(n, channels, plane, classes)) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(head::bwd_kernel<false>, dim3((unsigned)n), dim3(head::kT), 0, (hipStream_t)stream, dlogits, pooled,
                     weight, dh, slab_w, slab_b, channels, plane, classes, head::HeadSums{});
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_pool_linear_bwd_sums(const float* dlogits, const float* pooled, const float* weight, float* dh,
                                           float* slab_w, float* slab_b, const float* bn_y, const float* bn_out,
                                           const float* bn_mean, const float* bn_invstd, double* partial,
                                           int group_rows, int n, int channels, int plane, int classes, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!dlogits || !pooled || !weight || !dh || !head::ok(n, channels, plane, classes)) return (int)hipErrorInvalidValue;
  if (!bn_y || !bn_out || !bn_mean || !bn_invstd || !partial || plane != 64) return (int)hipErrorInvalidValue;
  if (group_rows < 0 || (group_rows > 0 && n % group_rows)) return (int)hipErrorInvalidValue;
  const head::HeadSums S = {bn_y, bn_out, bn_mean, bn_invstd, partial, group_rows};
  SGMCMC_LAUNCH(head::bwd_kernel<true>, dim3((unsigned)n), dim3(head::kT), 0, (hipStream_t)stream, dlogits, pooled,
                     weight, dh, slab_w, slab_b, channels, plane, classes, S);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_pool_linear_loss(const float* h, const float* weight, const float* bias, const int64_t* y,
                                       float* pooled, float* logits, float* dlogits, float* loss_rows, float* dh,
                                       float* slab_w, float* slab_b, const float* bn_y, const float* bn_out,
                                       const float* bn_mean, const float* bn_invstd, double* partial, int group_rows,
                                       int64_t* counters, int n_counters, int n, int channels, int plane, int classes,
                                       float grad_scale, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!h || !weight || !y || !pooled || !logits || !dlogits || !loss_rows || !dh || !head::ok(n, channels, plane, classes))
    return (int)hipErrorInvalidValue;
  if (counters && (n_counters <= 0 || n_counters > head::kT)) return (int)hipErrorInvalidValue;
  const bool sums = partial != nullptr;
  if (sums && (!bn_y || !bn_out || !bn_mean || !bn_invstd || plane != 64)) return (int)hipErrorInvalidValue;
  if (group_rows < 0 || (group_rows > 0 && n % group_rows)) return (int)hipErrorInvalidValue;
  const head::HeadSums S = {bn_y, bn_out, bn_mean, bn_invstd, partial, group_rows};
  if (sums)
    SGMCMC_LAUNCH(head::loss_kernel<true>, dim3((unsigned)n), dim3(head::kT), 0, (hipStream_t)stream, h, weight, bias, y,
                  pooled, logits, dlogits, loss_rows, dh, slab_w, slab_b, channels, plane, classes, grad_scale, S,
                  (long long*)counters, n_counters);
  else
    SGMCMC_LAUNCH(head::loss_kernel<false>, dim3((unsigned)n), dim3(head::kT), 0, (hipStream_t)stream, h, weight, bias, y,
                  pooled, logits, dlogits, loss_rows, dh, slab_w, slab_b, channels, plane, classes, grad_scale, S,
                  (long long*)counters, n_counters);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Softmax cross-entropy of the classifiers (models/base.py:168-191 through torch.distributions.Categorical;
// here: loss = scale * sum_b -log softmax(logits_b)[y_b]) in one launch each way instead of
// log_softmax + nll_loss and their two backward kernels.  One workgroup, one thread per row (<= 1024 rows,
// <= 16 classes); the row losses are summed in a fixed tree.
//   forward: probs[b,k] = softmax(logits_b)[k] (kept for the backward), loss[0] = scale * sum_b loss_b
//   backward: dlogits[b,k] = g * scale * (probs[b,k] - [k == y_b]),  g = *grad_out (a device scalar)
namespace xent {

// GRAD: instead of the probabilities the kernel leaves d loss / d logits = gscale * (p - onehot) -- exactly what
// bwd_kernel computes from the saved probabilities with grad_out * scale = gscale -- so a caller that seeds autograd
// itself (logits.backward(dlogits)) spends one launch on the likelihood instead of three (forward, ones, backward).
template <bool GRAD>
__global__ __launch_bounds__(1024) void fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y,
                                                   float* __restrict__ probs, float* __restrict__ loss, int B,
                                                   int K, float scale, float gscale) {
  __shared__ float sh[16];
  const int b = threadIdx.x;
  float l = 0.f;
  if (b < B) {
    float v[kMaxK];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) v[k] = logits[(size_t)b * K + k];
    l = row<kMaxK, GRAD>(v, K, y[b], gscale);      // (NaN for a label outside [0, K): the total is NaN then)
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) probs[(size_t)b * K + k] = v[k];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) l += __shfl_down(l, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = l;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += sh[w];
    loss[0] = tot * scale;
  }
}

__global__ __launch_bounds__(1024) void bwd_kernel(const float* __restrict__ probs, const int64_t* __restrict__ y,
                                                   const float* __restrict__ grad_out, float* __restrict__ dlogits,
                                                   int B, int K, float scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i % K;
  const float g = grad_out[0] * scale;
  dlogits[i] = g * (probs[i] - ((int64_t)k == y[b] ? 1.f : 0.f));      // (64-bit compare: the label rule of xent::row)
}

}  // namespace xent

extern "C" int sgmcmc_softmax_xent_fwd(const float* logits, const int64_t* y, float* probs, float* loss, int rows,
                                       int classes, double scale, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!logits || !y || !probs || !loss || rows <= 0 || rows > 1024 || classes <= 0 || classes > xent::kMaxK)
    return (int)hipErrorInvalidValue;
  const int threads = (rows + 63) & ~63;
  SGMCMC_LAUNCH(xent::fwd_kernel<false>, dim3(1), dim3((unsigned)threads), 0, (hipStream_t)stream, logits, y, probs,
                     loss, rows, classes, (float)scale, 0.f);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_softmax_xent_fwd_grad(const float* logits, const int64_t* y, float* loss, float* dlogits, int rows,
                                            int classes, double scale, float grad_scale, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!logits || !y || !dlogits || !loss || rows <= 0 || rows > 1024 || classes <= 0 || classes > xent::kMaxK)
    return (int)hipErrorInvalidValue;
  const int threads = (rows + 63) & ~63;
  SGMCMC_LAUNCH(xent::fwd_kernel<true>, dim3(1), dim3((unsigned)threads), 0, (hipStream_t)stream, logits, y, dlogits,
                     loss, rows, classes, (float)scale, grad_scale);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_softmax_xent_bwd(const float* probs, const int64_t* y, const float* grad_out, float* dlogits,
                                       int rows, int classes, double scale, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!probs || !y || !grad_out || !dlogits || rows <= 0 || classes <= 0) return (int)hipErrorInvalidValue;
  const int n = rows * classes;
  SGMCMC_LAUNCH(xent::bwd_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(1024), 0, (hipStream_t)stream, probs,
                     y, grad_out, dlogits, rows, classes, (float)scale);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- narrow linear layer
// y[n,k] = bias[k] + sum_j x[n,j] w[k,j] for a few outputs (K <= 16) and any width J: the classifier head of the
// convolutional net (Flatten -> Linear(2450, 10), models/conv_nets.py:57-70).  6 MFLOP at batch 128: a latency
// problem, not a GEMM -- one launch each way, every reduction in a fixed order (reproducible bit for bit), and no
// thread ever waits on one load at a time: a thread owns CH = 4 columns j per pass and issues its x loads and all
// K x CH weight loads of the pass before the first multiply.
//   forward : block = row n; a wave shuffle tree + the 4 waves in order finish the K sums.
//   backward: blocks [0, N): dx[n,j] = sum_k dy[n,k] w[k,j];  then ceil(J/256) x RG blocks: thread j sums
//             dy[n,k] x[n,j] over ITS row group (16 rows, 8 loads in flight) into slab [row group][k][j] -- the
//             caller adds the RG slabs in order (sgmcmc_wrw_reduce_many);  the last block: db[k] = sum_n dy[n,k].
namespace lin {

constexpr int KMAX = 16, CH = 4, ROWS_PER_GROUP = 16;

template <int K>
__device__ __forceinline__ void fwd_body(const float* __restrict__ x, const float* __restrict__ w,
                                         const float* __restrict__ bias, float* __restrict__ y, int J) {
  __shared__ float sh[4][KMAX];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* __restrict__ xr = x + (size_t)n * J;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;
  for (int j0 = tid; j0 < J; j0 += 256 * CH) {
    float xv[CH], wv[K][CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int j = j0 + 256 * c;
      xv[c] = j < J ? xr[j] : 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) wv[k][c] = j < J ? w[(size_t)k * J + j] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = fmaf(xv[c], wv[k][c], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) sh[wave][k] = v;
  }
  __syncthreads();
  if (tid < K) y[(size_t)n * K + tid] = ((sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid])) + (bias ? bias[tid] : 0.f);
}

template <int K>
__global__ __launch_bounds__(256) void fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                  const float* __restrict__ bias, float* __restrict__ y, int J) {
  fwd_body<K>(x, w, bias, y, J);
}

// ... and, in the same launch, the row's softmax cross-entropy on those logits (xent::fwd_kernel<GRAD>'s arithmetic, by
// thread 0 of the row's workgroup): dlogits[n,:] = gscale (softmax - onehot), loss_rows[n] = -log softmax[y_n].  The
// classifier's last layer and the likelihood in one launch instead of two at the launch floor (round 3).
template <int K>
__global__ __launch_bounds__(256) void fwd_loss_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, const int64_t* __restrict__ lab,
                                                       float* __restrict__ y, float* __restrict__ dlogits,
                                                       float* __restrict__ loss_rows, int J, float gscale) {
  fwd_body<K>(x, w, bias, y, J);
  __syncthreads();                       // (the row's logits: written by threads 0 .. K-1 of this workgroup)
  if (threadIdx.x == 0) {
    const int n = blockIdx.x;
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = y[(size_t)n * K + k];
    loss_rows[n] = xent::row<K, true>(v, K, lab[n], gscale);
#pragma unroll
    for (int k = 0; k < K; ++k) dlogits[(size_t)n * K + k] = v[k];
  }
}

template <int K>
__global__ __launch_bounds__(256) void bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                  const float* __restrict__ dy, float* __restrict__ dx,
                                                  float* __restrict__ dw_slabs, float* __restrict__ db, int N, int J) {
  __shared__ float dys[ROWS_PER_GROUP * KMAX];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int jb = (J + 255) / 256, rg = (N + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP;
  if (b < N) {
    if (!dx) return;
    float d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = dy[(size_t)b * K + k];
    for (int j0 = tid; j0 < J; j0 += 256 * CH) {
      float wv[K][CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int j = j0 + 256 * c;
#pragma unroll
        for (int k = 0; k < K; ++k) wv[k][c] = j < J ? w[(size_t)k * J + j] : 0.f;
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int j = j0 + 256 * c;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) v = fmaf(d[k], wv[k][c], v);
        if (j < J) dx[(size_t)b * J + j] = v;
      }
    }
  } else if (b < N + jb * rg) {
    if (!dw_slabs) return;
    const int g = (b - N) / jb, j = ((b - N) % jb) * 256 + tid;
    const int n0 = g * ROWS_PER_GROUP, n1 = min(N, n0 + ROWS_PER_GROUP);
    if (tid < (n1 - n0) * K) dys[tid] = dy[(size_t)n0 * K + tid];
    __syncthreads();
    if (j >= J) return;
    float xv[ROWS_PER_GROUP];
#pragma unroll
    for (int r = 0; r < ROWS_PER_GROUP; ++r) xv[r] = n0 + r < n1 ? x[(size_t)(n0 + r) * J + j] : 0.f;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
#pragma unroll
    for (int r = 0; r < ROWS_PER_GROUP; ++r) {
      if (n0 + r < n1) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = fmaf(dys[r * K + k], xv[r], acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) dw_slabs[((size_t)g * K + k) * J + j] = acc[k];
  } else if (db) {
    // db[k] = sum_n dy[n, k].  (One thread per k walking the N rows was a chain of N dependent trips to L2 -- 128 x
    // ~75 ns: this ONE workgroup was the whole launch's duration, 10 us.)  16 row classes per k: thread (k, r) adds rows
    // r, r + 16, ... (independent loads), then thread k adds its 16 partials in order.
    __shared__ float pdb[16][KMAX];
    const int k = tid & 15, r = tid >> 4;
    float v = 0.f;
    if (k < K) {
#pragma unroll 8
      for (int n = r; n < N; n += 16) v += dy[(size_t)n * K + k];
    }
    pdb[r][k] = v;
    __syncthreads();
    if (tid < K) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) t += pdb[q][tid];
      db[tid] = t;
    }
  }
}

}  // namespace lin

// K is a template parameter (the loads of a pass are issued together only with a compile-time trip count)
#define SGMCMC_LIN_DISPATCH(K_, CALL)                                                                        \
  switch (K_) {                                                                                              \
    case 1: { constexpr int KK = 1; CALL; break; }   case 2: { constexpr int KK = 2; CALL; break; }          \
    case 3: { constexpr int KK = 3; CALL; break; }   case 4: { constexpr int KK = 4; CALL; break; }          \
    case 5: { constexpr int KK = 5; CALL; break; }   case 6: { constexpr int KK = 6; CALL; break; }          \
    case 7: { constexpr int KK = 7; CALL; break; }   case 8: { constexpr int KK = 8; CALL; break; }          \
    case 9: { constexpr int KK = 9; CALL; break; }   case 10: { constexpr int KK = 10; CALL; break; }        \
    case 11: { constexpr int KK = 11; CALL; break; } case 12: { constexpr int KK = 12; CALL; break; }        \
    case 13: { constexpr int KK = 13; CALL; break; } case 14: { constexpr int KK = 14; CALL; break; }        \
    case 15: { constexpr int KK = 15; CALL; break; } default: { constexpr int KK = 16; CALL; break; }        \
  }

extern "C" int sgmcmc_linear_fwd(const float* x, const float* weight, const float* bias, float* y, int n, int in_features,
                                 int out_features, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !weight || !y || n <= 0 || in_features <= 0 || out_features <= 0 || out_features > lin::KMAX)
    return (int)hipErrorInvalidValue;
  SGMCMC_LIN_DISPATCH(out_features, SGMCMC_LAUNCH(lin::fwd_kernel<KK>, dim3((unsigned)n), dim3(256), 0,
                                                  (hipStream_t)stream, x, weight, bias, y, in_features));
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_linear_fwd_loss(const float* x, const float* weight, const float* bias, const int64_t* y_labels,
                                      float* y, float* dlogits, float* loss_rows, int n, int in_features,
                                      int out_features, float grad_scale, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !weight || !y || !y_labels || !dlogits || !loss_rows || n <= 0 || in_features <= 0 || out_features <= 0 ||
      out_features > lin::KMAX)
    return (int)hipErrorInvalidValue;
  SGMCMC_LIN_DISPATCH(out_features, SGMCMC_LAUNCH(lin::fwd_loss_kernel<KK>, dim3((unsigned)n), dim3(256), 0,
                                                  (hipStream_t)stream, x, weight, bias, y_labels, y, dlogits, loss_rows,
                                                  in_features, grad_scale));
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_linear_row_groups(int n) {
  return n <= 0 ? -1 : (n + lin::ROWS_PER_GROUP - 1) / lin::ROWS_PER_GROUP;
}

extern "C" int sgmcmc_linear_bwd(const float* x, const float* weight, const float* dy, float* dx, float* dweight_slabs,
                                 float* dbias, int n, int in_features, int out_features, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !weight || !dy || n <= 0 || in_features <= 0 || out_features <= 0 || out_features > lin::KMAX)
    return (int)hipErrorInvalidValue;
  const int rg = (n + lin::ROWS_PER_GROUP - 1) / lin::ROWS_PER_GROUP;
  const int blocks = n + ((in_features + 255) / 256) * rg + 1;
  SGMCMC_LIN_DISPATCH(out_features, SGMCMC_LAUNCH(lin::bwd_kernel<KK>, dim3((unsigned)blocks), dim3(256), 0,
                                                  (hipStream_t)stream, x, weight, dy, dx, dweight_slabs, dbias, n,
                                                  in_features));
  return (int)hipGetLastError();
}
