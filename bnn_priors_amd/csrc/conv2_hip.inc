// Persistent 3x3 / stride 1 / pad 1 convolutions of the ResNet trunk, second generation (round 3).
// Same contractions as conv_hip.inc (fp32 MFMA 16x16x4, exact f32), reorganised around what the round-2 profiles
// showed -- a launch was load -> MFMA -> store with nothing overlapped, every workgroup re-staged a 16 x 9C weight slab
// through LDS (the data gradient with 9C scalar gathers per 16 outputs), and the workgroups that share an image's
// input were spread over all eight XCDs (2.6-3.9x the algorithmic HBM reads at 64 channels):
//
//   * ITEMS of 4 image rows; 1024 items per launch for all three trunk shapes (16@32^2, 32@16^2, 64@8^2), 12 KiB of
//     input each.  A workgroup is PERSISTENT: it owns one tile of 16 output channels and walks its items; the next
//     item's input band is loaded into registers while the matrix pipe works on the current one (one LDS buffer, the
//     registers are the second one), so only the first load and the last store of a workgroup are exposed;
//   * the B operands (weights) never touch LDS: `weight_frag_kernel` leaves every convolution's weights in MFMA
//     fragment order once per gradient evaluation (forward order AND transposed + flipped for the data gradient), a
//     wave loads its 36 / 72 registers with coalesced 16-byte loads once per LAUNCH;
//   * 64 channels at 8x8: an item has two pixel tiles, so the four waves split K (input channels) in halves and the
//     halves are added through LDS in a fixed order -- 72 MFMAs per wave and item for every shape;
//   * XCD-aware item order: item j lives on XCD j mod 8 for every kernel of the trunk, and an image's bands, its
//     output-channel tiles, its data-gradient and its weight-gradient items all have the same j mod 8 -- what one
//     workgroup pulled into that XCD's L2 is what its neighbours need;
//   * LDS channel strides chosen per access pattern so that every ds_read_b32 of an MFMA operand is conflict free
//     (16 mod 32 for 16-pixel runs, 8 mod 32 for the 2 x 8 runs of the 8x8 stage, 2 mod 32 where the 16 n-lanes index
//     channels: the weight gradient).
//   * backward = ONE launch of 256 data-gradient + 256 weight-gradient workgroups, all persistent over 4 items
//     (equal MFMA work), weight-gradient accumulators live in registers across a workgroup's items: 256 / CT slabs
//     per output-channel tile instead of one per two items.
//
// Reference: the gradient of R1 (inference.py:215-223) through models/google_resnet.py:11-43.

#ifndef CONV2_STAMP
#define CONV2_STAMP(k)      /* the standalone lab (tools/conv_lab) defines this to record wall-clock stamps */
#endif

namespace conv2 {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using conv::BwdEpilogue;

constexpr int kXcd = 8;

// item j -> (image, band): XCD j % 8 owns images = j % 8 (mod 8); k = j / 8 walks (image group, band)
template <int BANDS>
__device__ __forceinline__ bool item_of(int j, int n_img, int& img, int& band) {
  const int k = j / kXcd;
  band = k % BANDS;
  img = kXcd * (k / BANDS) + j % kXcd;
  return img < n_img;
}
__host__ __device__ __forceinline__ int padded_items(int n_img, int bands) { return ((n_img + kXcd - 1) / kXcd) * kXcd * bands; }

template <int C, int HW, int ROWS>
struct Cfg {
  static constexpr int WP = HW + 8, ROWSH = ROWS + 2;
  static constexpr int CS_RAW = ROWSH * WP;
  static constexpr int WANT = HW >= 16 ? 16 : 8;
  static constexpr int CS = CS_RAW + ((WANT - CS_RAW % 32) % 32 + 32) % 32;
  static constexpr int CT = C / 16, BANDS = HW / ROWS;
  static constexpr int PT = ROWS * HW / 16;            // pixel tiles of an item
  static constexpr int KS = PT >= 4 ? 1 : 4 / PT;      // waves sharing one pixel tile (K split)
  static constexpr int PT_W = PT >= 4 ? PT / 4 : 1;    // pixel tiles per wave
  static constexpr int KK = C / 4 / KS;                // groups of 4 input channels per wave
  static constexpr int QW = 9 * KK;                    // k-steps = B registers per wave
  static constexpr int V = HW / 4;
  static constexpr int IN_V = C * ROWSH * V;           // float4 of an item's input band
  static constexpr int NV = (IN_V + 255) / 256;
  static constexpr int RED = KS > 1 ? 2 * 4 * 256 : 0; // floats: accumulator exchange of the K split (per item parity)
  static constexpr int SCR = 2 * 128;                  // floats: the waves' epilogue partials (per item parity)
  static constexpr size_t LDS_BYTES = (size_t)(2 * C * CS + RED + SCR) * sizeof(float);   // two band buffers
  static constexpr int FRAG = 9 * C * 16;              // floats of one output-channel tile's fragments
  static_assert(QW % 4 == 0 && (PT >= 4 ? PT % 4 == 0 : 4 % PT == 0) && CS % 4 == 0, "tile geometry");
};

// ---------------------------------------------------------------- weights in MFMA fragment order
// frag[ct][h][q4][lane] (float4; component j <-> k-step qi = 4 q4 + j of the wave's QW): rs = qi / KK, k2 = qi % KK,
// channel = 4 (h KK + k2) + (lane >> 4), n = lane & 15:
//   forward        B = w[ct*16 + n][channel][rs]
//   data gradient  B = w[channel][ct*16 + n][8 - rs]     (transposed, taps flipped)
struct FragJob { const float* w; float* fwd; float* dgrad; int channels; int ks; };
struct FragJobs { FragJob job[SGMCMC_FRAG_JOBS]; int first_block[SGMCMC_FRAG_JOBS + 1]; int n; };

__global__ __launch_bounds__(256) void weight_frag_kernel(FragJobs J) {
  int j = 0;
  while (j + 1 < J.n && (int)blockIdx.x >= J.first_block[j + 1]) ++j;
  const FragJob q = J.job[j];
  const int C = q.channels, KS = q.ks, KK = C / 4 / KS, QW = 9 * KK;
  const int e = ((int)blockIdx.x - J.first_block[j]) * 256 + (int)threadIdx.x;      // output float index
  if (e >= 9 * C * C) return;
  const int comp = e & 3, lane = (e >> 2) & 63, rest = e >> 8;                       // rest = (ct*KS + h) * (QW/4) + q4
  const int q4 = rest % (QW / 4), h = (rest / (QW / 4)) % KS, ct = rest / (QW / 4) / KS;
  const int qi = 4 * q4 + comp, rs = qi / KK, k2 = qi % KK;
  const int ch = 4 * (h * KK + k2) + (lane >> 4), n = ct * 16 + (lane & 15);
  if (q.fwd) q.fwd[e] = q.w[((size_t)n * C + ch) * 9 + rs];
  if (q.dgrad) q.dgrad[e] = q.w[((size_t)ch * C + n) * 9 + (8 - rs)];
}

// The same fragments four at a time, for workgroups that TRAIL another kernel's grid (convstem::fwd_frags_kernel: the
// preparation costs no launch): block `blk` of job q writes float4 blk * 256 + tid of each buffer -- the four k-steps of
// one (tile, half, q4, lane) -- so a job is ceil(9 C^2 / 1024) blocks, 243 for googleresnet's 16 convolutions.
__host__ __device__ __forceinline__ int frag_blocks4(int channels) { return (9 * channels * channels / 4 + 255) / 256; }
__device__ __forceinline__ void frag_block4(const FragJob& q, int blk) {
  const int C = q.channels, KS = q.ks, KK = C / 4 / KS, QW = 9 * KK;
  const int v = blk * 256 + (int)threadIdx.x;                                        // output float4 index
  if (4 * v >= 9 * C * C) return;
  const int lane = v & 63, rest = v >> 6;
  const int q4 = rest % (QW / 4), h = (rest / (QW / 4)) % KS, ct = rest / (QW / 4) / KS;
  const int n = ct * 16 + (lane & 15);
  float f[4], d[4];
#pragma unroll
  for (int comp = 0; comp < 4; ++comp) {
    const int qi = 4 * q4 + comp, rs = qi / KK, k2 = qi % KK;
    const int ch = 4 * (h * KK + k2) + (lane >> 4);
    f[comp] = q.fwd ? q.w[((size_t)n * C + ch) * 9 + rs] : 0.f;
    d[comp] = q.dgrad ? q.w[((size_t)ch * C + n) * 9 + (8 - rs)] : 0.f;
  }
  if (q.fwd) reinterpret_cast<float4*>(q.fwd)[v] = make_float4(f[0], f[1], f[2], f[3]);
  if (q.dgrad) reinterpret_cast<float4*>(q.dgrad)[v] = make_float4(d[0], d[1], d[2], d[3]);
}
// sgmcmc_frag_job[n] (n <= SGMCMC_FRAG_JOBS) -> FragJobs with `blocks_of(channels)` blocks per job; -> 0 or the refusal
template <typename BlocksOf>
inline int frag_jobs_from_abi(const sgmcmc_frag_job* jobs, int n, BlocksOf blocks_of, FragJobs& J) {
  J.n = n;
  int blocks = 0;
  for (int j = 0; j < n; ++j) {
    const sgmcmc_frag_job& q = jobs[j];
    const int c = q.channels;
    if (!q.w || (!q.fwd && !q.dgrad) || !(c == 16 || c == 32 || c == 64)) return (int)hipErrorInvalidValue;
    J.job[j] = {q.w, q.fwd, q.dgrad, c, c == 64 ? 2 : 1};      // K split of the 8x8 stage (Cfg::KS)
    J.first_block[j] = blocks;
    blocks += blocks_of(c);
  }
  J.first_block[n] = blocks;
  return 0;
}

// ---------------------------------------------------------------- epilogue reductions without a barrier of their own
// A wave leaves ITS per-channel partials in LDS right after its MFMAs (channel n lives in lanes n, n+16, n+32, n+48:
// fixed xor tree); the four waves' partials are combined -- in wave order, in double -- by threads 0..15 AFTER the
// barrier the next item needs anyway (or the one closing the launch).  scr: [wave][16][2] floats per item parity.
// STATS: (sum, M2 about the wave's OWN mean); the combination is Chan's parallel-variance formula, so nothing ever
// cancels against mean^2.  n_w = elements per channel held by one final wave.
template <int NT>
__device__ __forceinline__ void wave_stats(const f32x4 (&vals)[NT], bool active, float* __restrict__ scr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float s1 = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) s1 += (vals[t][0] + vals[t][1]) + (vals[t][2] + vals[t][3]);
  s1 += __shfl_xor(s1, 16, 64);
  s1 += __shfl_xor(s1, 32, 64);
  const float mean = s1 / (float)(NT * 16);
  float s2 = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float d0 = vals[t][0] - mean, d1 = vals[t][1] - mean, d2 = vals[t][2] - mean, d3 = vals[t][3] - mean;
    s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  s2 += __shfl_xor(s2, 16, 64);
  s2 += __shfl_xor(s2, 32, 64);
  if (lane < 16) *reinterpret_cast<float2*>(scr + (wave * 16 + lane) * 2) = active ? make_float2(s1, s2) : make_float2(0.f, 0.f);
}
// threads 0..15: (sum, M2) of channel tid over the item from the waves' pairs; `fin_mask` bit w = wave w holds values
__device__ __forceinline__ void combine_stats(const float* __restrict__ scr, unsigned fin_mask, int n_w,
                                              double* __restrict__ dst, size_t stride) {
  const int c = threadIdx.x;
  double S = 0.0, N = 0.0;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (fin_mask >> w & 1) { S += (double)scr[(w * 16 + c) * 2]; N += n_w; }
  const double mean = S / N;
  double M2 = 0.0;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (fin_mask >> w & 1) {
      // M2 about the wave's exact mean from the deviations about its float-rounded one, then Chan
      const double sw = (double)scr[(w * 16 + c) * 2], mw = sw / n_w, mr = (double)((float)sw / (float)n_w);
      const double d = mw - mean, dm = mw - mr;
      M2 += ((double)scr[(w * 16 + c) * 2 + 1] - n_w * dm * dm) + n_w * d * d;
    }
  dst[(size_t)c * stride] = S;
  dst[(size_t)c * stride + 1] = M2;
}
__device__ __forceinline__ void wave_sums(float s1, float s2, bool active, float* __restrict__ scr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  s1 += __shfl_xor(s1, 16, 64); s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 16, 64); s2 += __shfl_xor(s2, 32, 64);
  if (lane < 16) *reinterpret_cast<float2*>(scr + (wave * 16 + lane) * 2) = active ? make_float2(s1, s2) : make_float2(0.f, 0.f);
}
__device__ __forceinline__ void combine_sums(const float* __restrict__ scr, double* __restrict__ dst, size_t stride) {
  const int c = threadIdx.x;
  dst[(size_t)c * stride] = ((double)scr[c * 2] + (double)scr[(16 + c) * 2]) + ((double)scr[(32 + c) * 2] + (double)scr[(48 + c) * 2]);
  dst[(size_t)c * stride + 1] =
      ((double)scr[c * 2 + 1] + (double)scr[(16 + c) * 2 + 1]) + ((double)scr[(32 + c) * 2 + 1] + (double)scr[(48 + c) * 2 + 1]);
}

// ---------------------------------------------------------------- forward / data gradient
// wg of n_wg persistent workgroups (n_wg % (8 CT) == 0): output-channel tile ct = (wg / 8) % CT, item stream
// s = wg % 8 + 8 * (wg / (8 CT)) of n_wg / CT streams.  y[n, ct*16 + .., p] = sum_k x[n, k, p + tap] B[k], B from `frag`
// (forward or data-gradient fragments of weight_frag_kernel).  Epilogues as conv::conv3x3_body: STATS (batch
// statistics of the item for the BatchNorm that follows), EPI (+= e_dout [e_out > 0]), SUMS (partial sums of the
// BatchNorm backward that consumes the output); slice = img * BANDS + band of n_img * BANDS.
// ONE barrier per item (two with the K split of the 8x8 stage): the input band is double-buffered in LDS, the
// epilogue's cross-wave reductions are finished after the next item's barrier.
// LAB (tools/conv_lab only; 0 in the product): 1 = no MFMA loop, 2 = no input loads, 4 = no output stores
template <int C, int HW, int ROWS, bool STATS, bool EPI, bool SUMS, int LAB = 0>
__device__ __forceinline__ void conv_body(int wg, int n_wg, const float* __restrict__ x, const float* __restrict__ frag,
                                          float* __restrict__ y, double* __restrict__ stats, int n_img,
                                          const BwdEpilogue* E) {
  using G = Cfg<C, HW, ROWS>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* __restrict__ red = lds + 2 * C * G::CS;
  float* __restrict__ scr = lds + 2 * C * G::CS + G::RED;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, kq = lane >> 4;
  const int ct = (wg / kXcd) % G::CT;
  const int stream = wg % kXcd + kXcd * (wg / (kXcd * G::CT));
  const int n_streams = n_wg / G::CT;
  const int n_items = padded_items(n_img, G::BANDS);
  const int n_slices = n_img * G::BANDS;
  const int h = G::KS > 1 ? wave % G::KS : 0;                 // K split index of this wave
  const int pg = G::KS > 1 ? wave / G::KS : wave;             // pixel tile (group) of this wave
  const bool fin = h == 0;                                    // this wave ends up with final values
  constexpr unsigned FIN_MASK = G::KS == 1 ? 0xFu : (G::KS == 2 ? 0x5u : 0x1u);

  auto load_item = [&](int j, float4 (&r)[G::NV]) {
    int img, band;
    const bool ok = item_of<G::BANDS>(j, n_img, img, band);
    const float* __restrict__ xi = x + (size_t)img * C * HW * HW;
    const int y0 = band * ROWS;
#pragma unroll
    for (int it = 0; it < G::NV; ++it) {
      const int i = tid + it * 256;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((G::IN_V % 256 == 0) || i < G::IN_V) {
        const int v = i % G::V, ry = (i / G::V) % G::ROWSH, ci = i / (G::V * G::ROWSH);
        const int gy = y0 - 1 + ry;
        if (!(LAB & 2) && ok && gy >= 0 && gy < HW) val = *reinterpret_cast<const float4*>(xi + ((size_t)ci * HW + gy) * HW + 4 * v);
      }
      r[it] = val;
    }
  };
  auto store_item = [&](const float4 (&r)[G::NV], float* __restrict__ dst) {
#pragma unroll
    for (int it = 0; it < G::NV; ++it) {
      const int i = tid + it * 256;
      if ((G::IN_V % 256 == 0) || i < G::IN_V) {
        const int v = i % G::V, ry = (i / G::V) % G::ROWSH, ci = i / (G::V * G::ROWSH);
        *reinterpret_cast<float4*>(dst + ci * G::CS + ry * G::WP + 4 + 4 * v) = r[it];
      }
    }
  };

  CONV2_STAMP(0);
  float4 pre[G::NV];
  if (stream < n_items) load_item(stream, pre);
  // ---- this workgroup's B fragments (one output-channel tile, all K splits): global -> LDS once, then each wave
  // takes its registers from there (four waves loading the same 18-36 KB from L2 cost 1-1.5 us of a 10 us launch)
  float breg[G::QW];
  {
    constexpr int FV = G::KS * G::QW * 64 / 4, NF = (FV + 255) / 256;       // float4 of the tile's fragments
    static_assert(NF * 256 * 4 <= 2 * C * G::CS, "fragments are staged in the (still empty) band buffers");
    const float4* __restrict__ f4 = reinterpret_cast<const float4*>(frag) + (size_t)ct * FV;
    float4 fr[NF];
#pragma unroll
    for (int it = 0; it < NF; ++it) { const int i = tid + it * 256; fr[it] = f4[i < FV ? i : FV - 1]; }   // (all in flight together)
#pragma unroll
    for (int it = 0; it < NF; ++it) *reinterpret_cast<float4*>(lds + 4 * (tid + it * 256)) = fr[it];   // (no guard: no branch)
    __syncthreads();
    const float4* __restrict__ l4 = reinterpret_cast<const float4*>(lds) + (size_t)h * (G::QW / 4) * 64 + lane;
#pragma unroll
    for (int q4 = 0; q4 < G::QW / 4; ++q4) {
      const float4 b = l4[q4 * 64];
      breg[4 * q4] = b.x; breg[4 * q4 + 1] = b.y; breg[4 * q4 + 2] = b.z; breg[4 * q4 + 3] = b.w;
    }
    __syncthreads();
  }
  // halo columns (x = -1 and x = HW) of both buffers: zero once, item stores only touch the interior
  for (int i = tid; i < 2 * C * G::ROWSH * 2; i += 256) {
    const int side = i & 1, ry = (i >> 1) % G::ROWSH, ci = ((i >> 1) / G::ROWSH) % C, bufi = (i >> 1) / (G::ROWSH * C);
    lds[bufi * C * G::CS + ci * G::CS + ry * G::WP + (side ? HW + 4 : 3)] = 0.f;
  }
  // ---- geometry of this wave's pixel tiles (constant over items)
  int abase[G::PT_W], orow[G::PT_W], ocol[G::PT_W];
#pragma unroll
  for (int t = 0; t < G::PT_W; ++t) {
    const int p = pg * G::PT_W + t;
    int yy, x0, m_y, m_x;
    if (HW >= 16) { constexpr int TPR = HW >= 16 ? HW / 16 : 1; yy = p / TPR; x0 = (p % TPR) * 16; m_y = 0; m_x = n; }
    else { yy = 2 * p; x0 = 0; m_y = n >> 3; m_x = n & 7; }
    abase[t] = (4 * h * G::KK + kq) * G::CS + (yy + m_y) * G::WP + x0 + m_x + 3;
    const int m0 = 4 * kq;
    if (HW >= 16) { orow[t] = yy; ocol[t] = x0 + m0; }
    else { orow[t] = yy + (m0 >> 3); ocol[t] = m0 & 7; }
  }

  int lab_it = 0, par = 0, prev_slice = -1;
  for (int j = stream; j < n_items; j += n_streams, ++lab_it, par ^= 1) {
    int img, band;
    const bool ok = item_of<G::BANDS>(j, n_img, img, band);      // (uniform over the workgroup)
    float* __restrict__ in_s = lds + par * C * G::CS;
    if (lab_it == 1) CONV2_STAMP(8);
    store_item(pre, in_s);
    __syncthreads();
    if (lab_it == 0) CONV2_STAMP(1);
    if (lab_it == 1) CONV2_STAMP(9);
    if (j + n_streams < n_items) load_item(j + n_streams, pre);  // in flight during this item's MFMAs
    if ((STATS || SUMS) && prev_slice >= 0 && tid < 16) {        // the previous item's partials: all four waves wrote
      const float* ps = scr + (par ^ 1) * 128;
      if (STATS) combine_stats(ps, FIN_MASK, G::PT_W * 16, stats + ((size_t)(ct * 16) * n_slices + prev_slice) * 2, (size_t)n_slices * 2);
      if (SUMS) combine_sums(ps, E->s_partial + ((size_t)(ct * 16) * n_slices + prev_slice) * 2, (size_t)n_slices * 2);
    }
    prev_slice = -1;
    if (!ok) continue;
    const int y0 = band * ROWS;
    // the epilogue's own operands: issued before the MFMA loop, consumed after it
    float4 ex[G::PT_W], ey[G::PT_W], sy[G::PT_W], so[G::PT_W];
    float s_mean = 0.f, s_invstd = 0.f;
    if ((EPI || SUMS) && fin) {
      const size_t cbase = ((size_t)img * C + ct * 16 + n) * HW * HW;
#pragma unroll
      for (int t = 0; t < G::PT_W; ++t) {
        const size_t off = cbase + (size_t)(y0 + orow[t]) * HW + ocol[t];
        if (EPI) {
          ex[t] = *reinterpret_cast<const float4*>(E->e_dout + off);
          ey[t] = E->e_out ? *reinterpret_cast<const float4*>(E->e_out + off) : make_float4(1.f, 1.f, 1.f, 1.f);
        }
        if (SUMS) {
          sy[t] = *reinterpret_cast<const float4*>(E->s_y + off);
          so[t] = *reinterpret_cast<const float4*>(E->s_out + off);
        }
      }
      if (SUMS) {
        const int go = conv::group_offset(E, img, C);
        s_mean = E->s_mean[go + ct * 16 + n]; s_invstd = E->s_invstd[go + ct * 16 + n];
      }
    }
    constexpr int NACC = G::PT_W == 1 ? 2 : G::PT_W;           // a single tile splits its K chain in two
    f32x4 acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!(LAB & 1)) {
      // the A operands of tap rs + 1 are fetched from LDS while the matrix pipe works on tap rs (the compiler's own
      // schedule waits for every pair of reads right before the two MFMAs that use them)
      float a_cur[G::KK][G::PT_W], a_nxt[G::KK][G::PT_W];
#pragma unroll
      for (int k2 = 0; k2 < G::KK; ++k2)
#pragma unroll
        for (int t = 0; t < G::PT_W; ++t) a_cur[k2][t] = in_s[abase[t] + 4 * k2 * G::CS];
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) {
        if (rs + 1 < 9) {
          const int r = (rs + 1) / 3, s = (rs + 1) % 3;
#pragma unroll
          for (int k2 = 0; k2 < G::KK; ++k2)
#pragma unroll
            for (int t = 0; t < G::PT_W; ++t) a_nxt[k2][t] = in_s[abase[t] + 4 * k2 * G::CS + r * G::WP + s];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k2 = 0; k2 < G::KK; ++k2) {
#pragma unroll
          for (int t = 0; t < G::PT_W; ++t) {
            const int ai = G::PT_W == 1 ? (k2 & 1) : t;
            acc[ai] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[k2][t], breg[rs * G::KK + k2], acc[ai], 0, 0, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k2 = 0; k2 < G::KK; ++k2)
#pragma unroll
          for (int t = 0; t < G::PT_W; ++t) a_cur[k2][t] = a_nxt[k2][t];
      }
    } else {
#pragma unroll
      for (int t = 0; t < G::PT_W; ++t) acc[t][0] = in_s[abase[t]] + breg[t];
    }
    if (lab_it == 0) CONV2_STAMP(2);
    if (lab_it == 1) CONV2_STAMP(10);
    f32x4 vals[G::PT_W];
#pragma unroll
    for (int t = 0; t < G::PT_W; ++t) vals[t] = G::PT_W == 1 ? acc[0] + acc[1] : acc[t];
    if (G::KS > 1) {     // K halves / quarters: the partner waves' tiles are added in wave order
      float* __restrict__ rp = red + par * 4 * 256;
      if (!fin) *reinterpret_cast<float4*>(rp + wave * 256 + 4 * lane) = make_float4(vals[0][0], vals[0][1], vals[0][2], vals[0][3]);
      __syncthreads();
      if (fin) {
#pragma unroll
        for (int q = 1; q < G::KS; ++q) {
          const float4 o = *reinterpret_cast<const float4*>(rp + (wave + q) * 256 + 4 * lane);
          vals[0][0] += o.x; vals[0][1] += o.y; vals[0][2] += o.z; vals[0][3] += o.w;
        }
      }
    }
    // ---- store: lane holds 4 consecutive pixels of channel ct*16 + n
    float z1 = 0.f, z2 = 0.f;
    if (lab_it == 1) { if (vals[0][0] == 4321.f) CONV2_STAMP(15); CONV2_STAMP(11); }
    if (fin) {
      float* __restrict__ yo = y + ((size_t)img * C + ct * 16 + n) * HW * HW;
#pragma unroll
      for (int t = 0; t < G::PT_W; ++t) {
        f32x4 v = vals[t];
        if (EPI) {
          v[0] += ey[t].x > 0.f ? ex[t].x : 0.f; v[1] += ey[t].y > 0.f ? ex[t].y : 0.f;
          v[2] += ey[t].z > 0.f ? ex[t].z : 0.f; v[3] += ey[t].w > 0.f ? ex[t].w : 0.f;
        }
        vals[t] = v;
        if (SUMS) {
          const float d0 = so[t].x > 0.f ? v[0] : 0.f, d1 = so[t].y > 0.f ? v[1] : 0.f;
          const float d2 = so[t].z > 0.f ? v[2] : 0.f, d3 = so[t].w > 0.f ? v[3] : 0.f;
          z1 += (d0 + d1) + (d2 + d3);
          z2 += (d0 * ((sy[t].x - s_mean) * s_invstd) + d1 * ((sy[t].y - s_mean) * s_invstd)) +
                (d2 * ((sy[t].z - s_mean) * s_invstd) + d3 * ((sy[t].w - s_mean) * s_invstd));
          if (E->mask_dx) v = f32x4{d0, d1, d2, d3};       // (what is stored is dz: conv_hip.inc, BwdEpilogue)
        }
        if (!(LAB & 4) || v[0] == 1234.5678f)
          sgmcmc_store4<32>(y, yo + (size_t)(y0 + orow[t]) * HW + ocol[t], v[0], v[1], v[2], v[3]);
      }
    }
    if (lab_it == 1) CONV2_STAMP(12);
    if (SUMS) wave_sums(z1, z2, fin, scr + par * 128);
    if (STATS) wave_stats<G::PT_W>(vals, fin, scr + par * 128);
    prev_slice = img * G::BANDS + band;                  // dense: padding items have no slice
    if (lab_it == 0) CONV2_STAMP(3);
    if (lab_it == 1) { if (z1 == 4321.f) CONV2_STAMP(15); CONV2_STAMP(13); }
  }
  if ((STATS || SUMS) && prev_slice >= 0) {              // the last item's partials
    __syncthreads();
    if (tid < 16) {
      const float* ps = scr + (par ^ 1) * 128;
      if (STATS) combine_stats(ps, FIN_MASK, G::PT_W * 16, stats + ((size_t)(ct * 16) * n_slices + prev_slice) * 2, (size_t)n_slices * 2);
      if (SUMS) combine_sums(ps, E->s_partial + ((size_t)(ct * 16) * n_slices + prev_slice) * 2, (size_t)n_slices * 2);
    }
  }
  CONV2_STAMP(4);
}

template <int C, int HW, int ROWS, bool STATS, int LAB = 0>
__global__ __launch_bounds__(256, 2) void fwd_kernel(const float* __restrict__ x, const float* __restrict__ frag,
                                                     float* __restrict__ y, double* __restrict__ stats, int n_img) {
  conv_body<C, HW, ROWS, STATS, false, false, LAB>((int)blockIdx.x, (int)gridDim.x, x, frag, y, stats, n_img, nullptr);
}

// ---------------------------------------------------------------- weight gradient
// dw[co,ci,r,s] = sum_{n,p} dy[n,co,p] x[n,ci,p+(r-1,s-1)]: M = co (A = dy), N = ci (B = x shifted), K = pixels.
// Persistent workgroup = output-channel tile ct over a stream of items; wave = (input-channel tile, pixel split);
// per 4-pixel k-step ONE A fetch feeds the 9 taps' MFMAs (own B fetch, own accumulator tile each).  The 9 tiles stay
// in registers over all of the workgroup's items; at the end the pixel splits are added through LDS and the
// workgroup writes ONE slab [r,s][co 16][ci C] (tap-major, 64-byte runs) at part[(ct * P + p)], P = n_wg / CT.
template <int C, int HW, int ROWS>
struct WCfg {
  static constexpr int WP = HW + 8, ROWSH = ROWS + 2;
  static constexpr int CS_RAW = ROWSH * WP;
  static constexpr int CS = CS_RAW + ((2 - CS_RAW % 32) % 32 + 32) % 32;    // n-lanes = channels: stride = 2 mod 32
  static constexpr int NPIX = ROWS * HW;
  static constexpr int DS = NPIX + 2;                                       // (NPIX is a multiple of 32)
  static constexpr int NCI = C / 16, PS = 4 / NCI;
  static constexpr int KSTEPS = NPIX / 4 / PS;
  static constexpr int CT = C / 16, BANDS = HW / ROWS;
  static constexpr int V = HW / 4;
  static constexpr int IN_V = C * ROWSH * V, NV = (IN_V + 255) / 256;
  static constexpr int DY_V = 16 * NPIX / 4, NDV = (DY_V + 255) / 256;
  static constexpr int SLAB = 9 * 16 * C;
  static constexpr size_t STAGE = (size_t)C * CS + 16 * DS, REDF = 4 * 9 * 256;      // one item's operands; x2: double-buffered
  static constexpr size_t LDS_BYTES = (2 * STAGE > REDF ? 2 * STAGE : REDF) * sizeof(float);
  static_assert(NPIX % 32 == 0 && 4 % NCI == 0 && KSTEPS >= 1, "tile geometry");
};

template <int C, int HW, int ROWS>
__device__ __forceinline__ void wrw_body(int wg, int n_wg, const float* __restrict__ x, const float* __restrict__ dy,
                                         float* __restrict__ part, int n_img) {
  using G = WCfg<C, HW, ROWS>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, kq = lane >> 4;
  const int ct = (wg / kXcd) % G::CT;
  const int stream = wg % kXcd + kXcd * (wg / (kXcd * G::CT));
  const int n_streams = n_wg / G::CT;
  const int n_items = padded_items(n_img, G::BANDS);
  const int cit = wave % G::NCI, ps = wave / G::NCI;

  auto load_item = [&](int j, float4 (&rx)[G::NV], float4 (&rd)[G::NDV]) {
    int img, band;
    const bool ok = item_of<G::BANDS>(j, n_img, img, band);
    const int y0 = band * ROWS;
    const float* __restrict__ xi = x + (size_t)img * C * HW * HW;
    const float* __restrict__ di = dy + (((size_t)img * C + ct * 16) * HW + y0) * HW;
#pragma unroll
    for (int it = 0; it < G::NV; ++it) {
      const int i = tid + it * 256;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((G::IN_V % 256 == 0) || i < G::IN_V) {
        const int v = i % G::V, ry = (i / G::V) % G::ROWSH, ci = i / (G::V * G::ROWSH);
        const int gy = y0 - 1 + ry;
        if (ok && gy >= 0 && gy < HW) val = *reinterpret_cast<const float4*>(xi + ((size_t)ci * HW + gy) * HW + 4 * v);
      }
      rx[it] = val;
    }
#pragma unroll
    for (int it = 0; it < G::NDV; ++it) {
      const int i = tid + it * 256;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (((G::DY_V % 256 == 0) || i < G::DY_V) && ok) {
        const int v = i % (G::NPIX / 4), co = i / (G::NPIX / 4);
        val = *reinterpret_cast<const float4*>(di + (size_t)co * HW * HW + 4 * v);
      }
      rd[it] = val;
    }
  };
  auto store_item = [&](const float4 (&rx)[G::NV], const float4 (&rd)[G::NDV], float* __restrict__ in_s, float* __restrict__ dy_s) {
    // (channel strides = 2 mod 32: 8-byte aligned, so the float4 goes as two 8-byte stores)
#pragma unroll
    for (int it = 0; it < G::NV; ++it) {
      const int i = tid + it * 256;
      if ((G::IN_V % 256 == 0) || i < G::IN_V) {
        const int v = i % G::V, ry = (i / G::V) % G::ROWSH, ci = i / (G::V * G::ROWSH);
        float2* d = reinterpret_cast<float2*>(in_s + ci * G::CS + ry * G::WP + 4 + 4 * v);
        d[0] = make_float2(rx[it].x, rx[it].y); d[1] = make_float2(rx[it].z, rx[it].w);
      }
    }
#pragma unroll
    for (int it = 0; it < G::NDV; ++it) {
      const int i = tid + it * 256;
      if ((G::DY_V % 256 == 0) || i < G::DY_V) {
        const int v = i % (G::NPIX / 4), co = i / (G::NPIX / 4);
        float2* d = reinterpret_cast<float2*>(dy_s + co * G::DS + 4 * v);
        d[0] = make_float2(rd[it].x, rd[it].y); d[1] = make_float2(rd[it].z, rd[it].w);
      }
    }
  };

  f32x4 acc[9];
#pragma unroll
  for (int rs = 0; rs < 9; ++rs) acc[rs] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 prx[G::NV], prd[G::NDV];
  if (stream < n_items) load_item(stream, prx, prd);
  for (int i = tid; i < 2 * C * G::ROWSH * 2; i += 256) {
    const int side = i & 1, ry = (i >> 1) % G::ROWSH, ci = ((i >> 1) / G::ROWSH) % C, bufi = (i >> 1) / (G::ROWSH * C);
    lds[bufi * G::STAGE + ci * G::CS + ry * G::WP + (side ? HW + 4 : 3)] = 0.f;
  }
  int par = 0;
  for (int j = stream; j < n_items; j += n_streams, par ^= 1) {
    float* __restrict__ in_s = lds + par * G::STAGE;
    float* __restrict__ dy_s = in_s + C * G::CS;
    const float* __restrict__ bsrc = in_s + (cit * 16 + n) * G::CS + kq + 3;
    const float* __restrict__ asrc = dy_s + n * G::DS + kq;
    store_item(prx, prd, in_s, dy_s);
    __syncthreads();           // the ONE barrier of an item: the other buffer is still being read by slower waves
    if (j + n_streams < n_items) load_item(j + n_streams, prx, prd);
    // (a padding item holds zeros: its MFMAs add nothing)
    // operands of k-step kk + 1 are fetched while the matrix pipe works on k-step kk
    float a_cur, b_cur[9], a_nxt = 0.f, b_nxt[9];
    auto fetch = [&](int kk, float& a, float (&b)[9]) {
      const int g = ps * G::KSTEPS + kk;              // 4-pixel group within the item
      const int row = g / G::V, xg = g % G::V;
      a = asrc[4 * g];
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) b[rs] = bsrc[(row + rs / 3) * G::WP + 4 * xg + rs % 3];
    };
    fetch(0, a_cur, b_cur);
#pragma unroll
    for (int kk = 0; kk < G::KSTEPS; ++kk) {
      if (kk + 1 < G::KSTEPS) fetch(kk + 1, a_nxt, b_nxt);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) acc[rs] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur, b_cur[rs], acc[rs], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      a_cur = a_nxt;
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) b_cur[rs] = b_nxt[rs];
    }
  }
  // ---- sum the pixel splits, write this workgroup's slab
  __syncthreads();
  float* __restrict__ red = lds;  // [wave][rs][256]
#pragma unroll
  for (int rs = 0; rs < 9; ++rs)
    *reinterpret_cast<float4*>(red + (wave * 9 + rs) * 256 + 4 * lane) = make_float4(acc[rs][0], acc[rs][1], acc[rs][2], acc[rs][3]);
  __syncthreads();
  const int P = n_streams;
  float* __restrict__ out = part + ((size_t)ct * P + stream) * G::SLAB;
  for (int i = tid; i < G::NCI * 9 * 256; i += 256) {
    const int e = i % 256, rs = (i / 256) % 9, ci_t = i / (256 * 9);
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < G::PS; ++q) v += red[((q * G::NCI + ci_t) * 9 + rs) * 256 + e];
    const int ln = e >> 2, vv = e & 3;               // D[row = 4*(ln>>4) + vv][col = ln & 15]
    const int co = 4 * (ln >> 4) + vv, ci = ci_t * 16 + (ln & 15);
    out[((size_t)rs * 16 + co) * C + ci] = v;
  }
}

// Both gradients of one convolution in ONE launch of persistent workgroups: blocks [0, n_wrw) accumulate weight-
// gradient slabs, blocks [n_wrw, gridDim) compute the data gradient (dgrad fragments); n_wrw % 8 == 0.
template <int C, int HW, int ROWS, bool EPI, bool SUMS>
__global__ __launch_bounds__(256, 2) void bwd_kernel(const float* __restrict__ x, const float* __restrict__ frag_dgrad,
                                                     const float* __restrict__ dy, float* __restrict__ dx,
                                                     float* __restrict__ part, int n_wrw, int n_img, BwdEpilogue E) {
  const int b = (int)blockIdx.x;
  if (b < n_wrw) wrw_body<C, HW, ROWS>(b, n_wrw, x, dy, part, n_img);
  else conv_body<C, HW, ROWS, false, EPI, SUMS>(b - n_wrw, (int)gridDim.x - n_wrw, dy, frag_dgrad, dx, nullptr, n_img, &E);
}

template <int C, int HW, int ROWS>
constexpr size_t bwd_lds() {
  return Cfg<C, HW, ROWS>::LDS_BYTES > WCfg<C, HW, ROWS>::LDS_BYTES ? Cfg<C, HW, ROWS>::LDS_BYTES : WCfg<C, HW, ROWS>::LDS_BYTES;
}

}  // namespace conv2

// ---------------------------------------------------------------- launchers + C ABI
namespace conv2 {

constexpr int kRows = 4;
constexpr int kMaxFwd = 512, kMaxHalf = 256;   // persistent grid: 2 workgroups per CU; backward = two halves of 256
// Launches that carry several minibatches run THREE workgroups per CU at 16 and 32 channels (what their LDS -- 31 - 50 KB --
// and registers -- <= 151 -- admit; the 64-channel kernels' 62 KB admit two).  The two workgroups of a CU run in lock-step
// (tools/conv_lab stamps at 512 images: per item 1.96 us in which their two waves per SIMD share the matrix pipe + 1.15 us
// of staging / epilogue with the pipe idle: 63 % busy; a deliberate half-period offset between them does not hold) -- a
// third wave per SIMD fills the gaps: forward 28.4 -> 26.4 us, backward 61.5 -> 54.4 / 56.1 -> 51.3 us at 512 images;
// at 128 images (1,024 items) it is slower.
constexpr int kBigImages = 256, kBigNum = 3;   // launches with >= 256 images run 3 / 2 times the persistent grid at <= 32 channels
template <int C>
__host__ inline int grid_cap(int cap, int n_img) {
  return (C <= 32 && n_img >= kBigImages) ? cap * kBigNum / 2 : cap;
}

template <int C, int HW>
int launch_fwd(const float* x, const float* frag, float* y, int n_img, double* stats, hipStream_t s) {
  using G = Cfg<C, HW, kRows>;
  auto k0 = fwd_kernel<C, HW, kRows, false>;
  auto k1 = fwd_kernel<C, HW, kRows, true>;
  static bool attr_done = false;
  if (!attr_done) {
    for (const void* k : {reinterpret_cast<const void*>(k0), reinterpret_cast<const void*>(k1)}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  const int want = padded_items(n_img, G::BANDS) * G::CT;      // (a multiple of 8 CT)
  const int cap = grid_cap<C>(kMaxFwd, n_img);
  const dim3 grid((unsigned)(want < cap ? want : cap)), block(256);
  if (stats) SGMCMC_LAUNCH(k1, grid, block, G::LDS_BYTES, s, x, frag, y, stats, n_img);
  else SGMCMC_LAUNCH(k0, grid, block, G::LDS_BYTES, s, x, frag, y, stats, n_img);
  return (int)hipGetLastError();
}

template <int C, int HW>
int half_grid(int n_img) {
  const int want = padded_items(n_img, HW / kRows) * (C / 16), cap = grid_cap<C>(kMaxHalf, n_img);
  return want < cap ? want : cap;
}

template <int C, int HW>
int launch_bwd(const float* x, const float* frag, const float* dy, float* dx, const BwdEpilogue& E, float* dw,
               float* part, int n_img, int* n_slabs, hipStream_t s) {
  using W = WCfg<C, HW, kRows>;
  constexpr size_t lds = bwd_lds<C, HW, kRows>();
  auto k00 = bwd_kernel<C, HW, kRows, false, false>;
  auto k10 = bwd_kernel<C, HW, kRows, true, false>;
  auto k01 = bwd_kernel<C, HW, kRows, false, true>;
  auto k11 = bwd_kernel<C, HW, kRows, true, true>;
  static bool attr_done = false;
  if (!attr_done) {
    for (const void* f : {reinterpret_cast<const void*>(k00), reinterpret_cast<const void*>(k10),
                          reinterpret_cast<const void*>(k01), reinterpret_cast<const void*>(k11)}) {
      const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  const int half = half_grid<C, HW>(n_img);
  const dim3 grid((unsigned)(2 * half)), block(256);
  const bool epi = E.e_dout != nullptr, sums = E.s_partial != nullptr;
  if (epi && sums) SGMCMC_LAUNCH(k11, grid, block, lds, s, x, frag, dy, dx, part, half, n_img, E);
  else if (epi) SGMCMC_LAUNCH(k10, grid, block, lds, s, x, frag, dy, dx, part, half, n_img, E);
  else if (sums) SGMCMC_LAUNCH(k01, grid, block, lds, s, x, frag, dy, dx, part, half, n_img, E);
  else SGMCMC_LAUNCH(k00, grid, block, lds, s, x, frag, dy, dx, part, half, n_img, E);
  const int P = half / (C / 16);
  conv::SlabSet tiles[C / 16];          // one slab set per 16-output-channel tile
  for (int t = 0; t < C / 16; ++t) tiles[t] = {part + (size_t)t * P * W::SLAB, W::SLAB, dw + (size_t)t * W::SLAB, 9};
  return conv::finish_slabs(n_slabs, P, s, tiles, C / 16);
}

}  // namespace conv2

extern "C" int sgmcmc_conv3x3_prepare_weights(const sgmcmc_frag_job* jobs, int n_jobs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!jobs || n_jobs <= 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  for (int base = 0; base < n_jobs; base += SGMCMC_FRAG_JOBS) {
    conv2::FragJobs J;
    const int n = n_jobs - base < SGMCMC_FRAG_JOBS ? n_jobs - base : SGMCMC_FRAG_JOBS;
    if (const int bad = conv2::frag_jobs_from_abi(jobs + base, n, [](int c) { return (9 * c * c + 255) / 256; }, J))
      return bad;
    SGMCMC_LAUNCH(conv2::weight_frag_kernel, dim3((unsigned)J.first_block[n]), dim3(256), 0, s, J);
  }
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_conv3x3_frag_stat_slices(int n_img, int channels, int hw) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!conv::is_trunk_shape(channels, hw) || n_img <= 0) return -1;
  return n_img * (hw / conv2::kRows);
}

extern "C" int64_t sgmcmc_conv3x3_frag_scratch_floats(int n_img, int channels, int hw) {
  if (!conv::is_trunk_shape(channels, hw) || n_img <= 0) return -1;
  const int half = channels == 16 ? conv2::half_grid<16, 32>(n_img) : channels == 32 ? conv2::half_grid<32, 16>(n_img)
                                                                                      : conv2::half_grid<64, 8>(n_img);
  return (int64_t)half * 144 * channels;
}

extern "C" int sgmcmc_conv3x3_frag_fwd(const float* x, const float* frag_fwd, float* y, int n_img, int channels, int hw,
                                       double* stats, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !frag_fwd || !y || n_img <= 0) return (int)hipErrorInvalidValue;
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv2::launch_fwd<C, HW>(x, frag_fwd, y, n_img, stats, (hipStream_t)stream));
}

extern "C" int sgmcmc_conv3x3_frag_bwd(const float* x, const float* frag_dgrad, const float* dy, float* dx,
                                       const sgmcmc_conv_bwd_epilogue* epi, float* dw, float* scratch, int n_img,
                                       int channels, int hw, int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !frag_dgrad || !dy || !dx || !scratch || n_img <= 0 || (!dw && !deferred_slabs)) return (int)hipErrorInvalidValue;
  conv::BwdEpilogue E{};
  if (epi)
    if (const int bad = conv::epilogue_from_abi(epi, n_img, E)) return bad;
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv2::launch_bwd<C, HW>(x, frag_dgrad, dy, dx, E, dw, scratch, n_img, deferred_slabs,
                                                                (hipStream_t)stream));
}

