// The convolutional classifier's second convolution: 50 -> 50 channels, 3x3 / stride 1 / pad 1 on 14x14 maps,
// NCHW fp32, no bias here (it joins sgmcmc_bias_relu_pool_*) -- models/conv_nets.py:46-70 inside the gradient
// evaluation of inference.py:215-223 -- as implicit GEMMs on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32).
//
// Neither 50 nor 14 is a multiple of a tile edge, so the tiling differs from the ResNet trunk's (conv_hip.inc):
//   * pixels: a tile is 16 consecutive pixels of the FLATTENED 14x14 plane (196 = 12 tiles + 4 pixels: 13 tiles,
//     6 % padding); a lane's 4 output pixels 16t + 4q .. +3 are contiguous in the plane, so results still leave
//     as one dwordx4 store per tile.  Every lane carries its own (row, column) LDS offset.
//   * output channels: 4 tiles of 16 (the last one 2 wide: its other columns multiply zero weights);
//   * K = (tap, input channel) with the channels padded to 52 IN LDS ONLY (two zero planes / zero weight columns):
//     9 x 13 = 117 k-steps of 4 channels of one tap, so a k-step's LDS offset is a compile-time constant.
// One workgroup = (image, PAIR of output-channel tiles), 512 threads: the whole image (50 planes with a one-pixel
// zero frame) and the 32 x 468 weight slab live in LDS (127 KB: one workgroup per CU, 256 workgroups at batch 128 --
// ONE round over the 256 CUs; with a workgroup per single tile the 512 workgroups took two rounds and staged the
// image four times instead of twice: 27.6 -> 22.2 us); a wave owns one channel tile and 3 - 4 pixel tiles (a B fetch
// feeds 3 - 4 MFMAs) -- two waves per SIMD, so one wave's LDS operand latency hides behind the other's MFMAs (with 4
// waves per CU the same kernel ran 2.5x slower: measured).  Operand staging is two-phase:
// every global load in flight before the first LDS store.
//
//   forward        y[n,co,p]   = sum_{ci,r,s} x[n,ci,p+(r-1,s-1)] w[co,ci,r,s]
//   data gradient  dx[n,ci,p]  = sum_{co,r,s} dy[n,co,p-(r-1,s-1)] w[co,ci,r,s]   = the forward body on dy with
//                  w'[ci,co,r,s] = w[co,ci,2-r,2-s] gathered while staging                         (TRANSPOSE_W)
//   weight gradient dw[co,ci,r,s] = sum_{n,p} dy[n,co,p] x[n,ci,p+(r-1,s-1)]: M = co tile, N = ci tile per tap,
//                  K = pixels (49 k-steps per image); workgroup = (2 images, co tile), wave = ci tile with nine
//                  accumulator tiles; per-workgroup partial slabs, fixed-order reduction (conv::wrw_reduce_*).

#ifndef CONV50_STAMP
#define CONV50_STAMP(k)      /* tools/conv_lab/lab50 defines this to record wall-clock stamps */
#endif

namespace conv50 {

using conv::f32x4;
constexpr int T = 512;                                             // threads per workgroup (8 waves)
constexpr int C = 50, CP = 52, HW = 14, NPIX = HW * HW, NT = 13;   // channels, padded; side; pixels; pixel tiles
constexpr int WP = 20, ROWS = HW + 2;                              // row pitch (data at columns 4..17), rows with frame
constexpr int K = 9 * CP, KSTEPS = CP / 4;                          // 468; 13 k-steps per tap
// weight rows in LDS: K ordered (channel, tap) AS IN MEMORY (a row is a straight copy), pitch = 2 mod 32 so that the 16
// n-lanes x 2 k-lanes of a B fetch (address n KP + 9 kq + const) fall on 32 different banks
constexpr int KP = 482;
constexpr int CT = 4;                                              // output-channel tiles
constexpr int NPAIR = 2, WROWS = 32;                               // forward / data gradient: two tiles per workgroup
// channel stride: forward / data gradient -- the 4 k-lanes of an A fetch read 4 channels: keep them half a bank
// row apart (stride = 16 mod 32); weight gradient -- the 16 n-lanes of a B fetch index channels (stride = 2 mod 32)
constexpr int CS_F = ROWS * WP + 16;                               // 336
constexpr int CS_W = ROWS * WP + 2;                                // 322: = 2 mod 32 (n-lanes = channels: banks 2n + k)
constexpr size_t LDS_F = (size_t)(CP * CS_F + WROWS * KP) * sizeof(float);
// (Round 4 measured (image, ONE channel tile, HALF of the rows) workgroups with K split over 8 waves -- two per CU at 74 KB
//  instead of one at 131 KB: conv_pool 19.7 -> 28.9 us, bwd_pool 37.8 -> 45.1 us, the co-resident workgroups ran in lock
//  step and the image was staged 8 times instead of 2.  Removed in round 6; docs/lab_notes.md keeps the numbers.)
constexpr int NSUB = NPAIR;                                        // forward / data-gradient workgroups per image
constexpr size_t LDS_FWD = LDS_F;
constexpr int DS = NPIX + 2;                                       // dy tile pitch (198 = 6 mod 32: banks 6n + k all distinct)
constexpr int ITEMS = 2;                                           // images per weight-gradient workgroup
constexpr int CPW = C + 1;                                         // weight gradient: ONE zero plane (columns >= 50 are discarded)
constexpr size_t LDS_W_STAGE = (size_t)(CPW * CS_W + 16 * DS + 2 + 16 * 49) * sizeof(float);   // 81,504 B: two per CU
constexpr size_t LDS_W_RED = (size_t)(4 * 9 * 256) * sizeof(float);   // one pixel half's accumulators
constexpr size_t LDS_W = LDS_W_STAGE > LDS_W_RED ? LDS_W_STAGE : LDS_W_RED;

template <int TOTAL, typename V, typename Ld>
__device__ __forceinline__ void stage_load(V (&r)[(TOTAL + T - 1) / T], Ld ld) {
#pragma unroll
  for (int it = 0; it < (TOTAL + T - 1) / T; ++it) {
    const int i = (int)threadIdx.x + it * T;
    if ((TOTAL % T == 0) || i < TOTAL) r[it] = ld(i);
  }
}
template <int TOTAL, typename V, typename St>
__device__ __forceinline__ void stage_store(const V (&r)[(TOTAL + T - 1) / T], St st) {
#pragma unroll
  for (int it = 0; it < (TOTAL + T - 1) / T; ++it) {
    const int i = (int)threadIdx.x + it * T;
    if ((TOTAL % T == 0) || i < TOTAL) st(i, r[it]);
  }
}

// the image: 50 planes x 14 rows x 7 float2 (a row is 56 B: 8-byte aligned whatever the row) -> LDS rows of pitch WP.
// (round 2 moved float4 and scattered their 4 elements with a row / column division each: 20 scalar LDS stores per
// thread behind ~15 integer instructions apiece -- half of a 5.8 us staging phase, tools/conv_lab/lab50.)
template <int CS, int PLANES = CP>
struct ImageStage {
  static constexpr int TOTAL = C * HW * (HW / 2), IT = (TOTAL + T - 1) / T;
  float2 r[IT];
  __device__ __forceinline__ void load(const float* __restrict__ xi) {
    stage_load<TOTAL, float2>(r, [&](int i) { return *reinterpret_cast<const float2*>(xi + 2 * (size_t)i); });
  }
  __device__ __forceinline__ void store(float* __restrict__ in_s) const {
    stage_store<TOTAL, float2>(r, [&](int i, const float2& q) {
      const int j = i % (HW / 2), row = (i / (HW / 2)) % HW, ci = i / (HW * (HW / 2));
      *reinterpret_cast<float2*>(in_s + ci * CS + (row + 1) * WP + 4 + 2 * j) = q;
    });
  }
  // the zero frame (rows 0 and 15, columns 3 and 18) and the two padding planes
  static __device__ __forceinline__ void zero_frame(float* __restrict__ in_s) {
    const int tid = threadIdx.x;
    for (int i = tid; i < C * 2 * WP; i += T) {              // top and bottom rows
      const int ci = i / (2 * WP), rr = (i / WP) % 2, col = i % WP;
      in_s[ci * CS + (rr ? ROWS - 1 : 0) * WP + col] = 0.f;
    }
    for (int i = tid; i < C * HW * 2; i += T) {              // left and right columns of the data rows
      const int ci = i / (HW * 2), row = (i / 2) % HW, side = i & 1;
      in_s[ci * CS + (row + 1) * WP + (side ? HW + 4 : 3)] = 0.f;
    }
    for (int i = tid; i < (PLANES - C) * CS; i += T) in_s[C * CS + i] = 0.f;
  }
};

// ---- the layer WITH its tail: conv -> + bias -> ReLU -> MaxPool2d(2) (conv_nets.py:58-66) --------------------------
// Forward: the 50 x 14 x 14 map stays in LDS; what leaves is the pooled 50 x 7 x 7 map and one byte per pooled element
// (bits 0-1: the window position of the first maximum in scan order, NaNs win, as ATen; bit 2: max + bias > 0).
// Backward: the gradient w.r.t. the 14 x 14 map exists only in LDS -- every 2 x 2 window is written whole (one
// non-zero at most) from the pooled gradient and that byte, for the data gradient's image (PooledStage) and for the
// weight gradient's 16-channel dy tile alike; the bias gradient's partial sums leave with the weight-gradient slabs.
constexpr int PH = HW / 2, PCELLS = PH * PH;                       // 7 x 7 pooled cells per plane
struct PoolArgs {
  const float* bias;          // forward epilogue
  float* pooled;
  uint8_t* code;
  const uint8_t* src_code;    // backward: the bytes that belong to the pooled gradient
  float* dbias_part;          // weight-gradient workgroups: [pair of images][50] partial sums (may be NULL)
};

template <int CS>
struct PooledStage {
  static constexpr int TOTAL = C * PCELLS, IT = (TOTAL + T - 1) / T;
  float d[IT];
  uint8_t k[IT];
  __device__ __forceinline__ void load(const float* __restrict__ dp, const uint8_t* __restrict__ cd) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = (int)threadIdx.x + it * T;
      d[it] = 0.f;
      k[it] = 0;
      if (i < TOTAL) { d[it] = dp[i]; k[it] = cd[i]; }
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ in_s) const {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = (int)threadIdx.x + it * T;
      if (i < TOTAL) {
        const int ci = i / PCELLS, cell = i % PCELLS, oi = cell / PH, oj = cell % PH;
        conv::unpool_window(in_s + ci * CS + (2 * oi + 1) * WP + 4 + 2 * oj, WP, d[it], k[it]);
      }
    }
  }
};

// ---------------------------------------------------------------- forward / data gradient
// wT (forward only, may be NULL): the workgroups also leave wT[ci][co][rs] = w[co][ci][8 - rs] -- the weights as the
// DATA GRADIENT wants them (its B rows contiguous), 88 elements per workgroup: the backward then stages its weights
// with the forward's straight copy instead of 28 strided gathers per thread (bwd_t_kernel).
// FROM_POOLED: the image is the gradient of a pooled map (x = that gradient, pa.src_code its bytes);
// POOL_EPI: the result leaves through + bias -> ReLU -> MaxPool2d(2) (pa.bias, pa.pooled, pa.code; y unused).
template <bool TRANSPOSE_W, bool FROM_POOLED = false, bool POOL_EPI = false>
__device__ __forceinline__ void conv_body(int b, int n_blocks, const float* __restrict__ x, const float* __restrict__ w,
                                          float* __restrict__ y, float* __restrict__ wT = nullptr,
                                          const PoolArgs pa = PoolArgs{nullptr, nullptr, nullptr, nullptr, nullptr}) {
  extern __shared__ float lds[];
  float* __restrict__ in_s = lds;
  float* __restrict__ w_s = lds + CP * CS_F;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pair = b % NPAIR, img = b / NPAIR;
  CONV50_STAMP(0);
  if (wT) {
    const int per = (C * C * 9 + n_blocks - 1) / n_blocks;
    for (int o = b * per + tid; o < (b + 1) * per && o < C * C * 9; o += T) {
      const int rs = o % 9, co = (o / 9) % C, ci = o / (9 * C);
      wT[o] = w[((size_t)co * C + ci) * 9 + (8 - rs)];
    }
  }
  {
    typename std::conditional<FROM_POOLED, PooledStage<CS_F>, ImageStage<CS_F>>::type im;
    auto load_image = [&]() {
      if constexpr (FROM_POOLED) im.load(x + (size_t)img * C * PCELLS, pa.src_code + (size_t)img * C * PCELLS);
      else im.load(x + (size_t)img * C * NPIX);
    };
    // weight slab: w_s[n][c * 9 + tap] for the 32 output channels n of this tile pair (zero rows beyond channel 49)
    if (!TRANSPOSE_W) {
      constexpr int NW2 = WROWS * (C * 9 / 2);              // 7200 float2: a row is 450 contiguous floats
      float2 rw[(NW2 + T - 1) / T];
      stage_load<NW2, float2>(rw, [&](int i) {
        const int n = i / (C * 9 / 2), co = pair * WROWS + n;
        float2 q = make_float2(0.f, 0.f);
        if (co < C) q = *reinterpret_cast<const float2*>(w + (size_t)co * (C * 9) + 2 * (i % (C * 9 / 2)));
        return q;
      });
      load_image();
      stage_store<NW2, float2>(rw, [&](int i, const float2& q) {
        *reinterpret_cast<float2*>(w_s + (i / (C * 9 / 2)) * KP + 2 * (i % (C * 9 / 2))) = q;
      });
    } else {
      // (stand-alone data gradient without a prepared wT) w'[n = ci_out][(co_in, tap)] = w[co_in][ci_out][8 - tap]
      constexpr int NW = WROWS * C * 9;
      float rw[(NW + T - 1) / T];
      stage_load<NW, float>(rw, [&](int i) {
        const int n = i / (C * 9), e = i % (C * 9), co = e / 9, rs = e % 9, cio = pair * WROWS + n;
        return cio < C ? w[((size_t)co * C + cio) * 9 + (8 - rs)] : 0.f;
      });
      load_image();
      stage_store<NW, float>(rw, [&](int i, float q) { w_s[(i / (C * 9)) * KP + i % (C * 9)] = q; });
    }
    for (int i = tid; i < WROWS * 9 * (CP - C); i += T)     // the two padding channels: K entries 450 .. 467 of every row
      w_s[(i / (9 * (CP - C))) * KP + C * 9 + i % (9 * (CP - C))] = 0.f;
    im.store(in_s);
    ImageStage<CS_F>::zero_frame(in_s);
  }
  __syncthreads();
  CONV50_STAMP(1);

  const int n = lane & 15, kq = lane >> 4;
  // 13 pixel tiles x 2 channel tiles = 26 tile units over 8 waves: wave w owns channel tile h = w & 1 (ONE B fetch per
  // k-step) and pixel tiles (w >> 1) + 4j, j = 0 .. 3 (4 of them for w < 2, else 3) -- 7 / 7 / 6 / 6 units per SIMD
  // (waves w and w + 4 share one), against 8 / 6 / 6 / 6 when a wave took both channel tiles of its pixel tiles.
  const int wv = __builtin_amdgcn_readfirstlane(wave);      // (scalar: the 4-tile / 3-tile choice is a scalar branch)
  const int h = wv & 1, t0 = wv >> 1;
  const bool four = t0 + 12 < NT;
  int abase[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int pix = 16 * (t0 + 4 * j) + n;
    if (pix >= NPIX) pix = 0;                               // padding rows of the last tile / no fourth tile: any valid address
    abase[j] = kq * CS_F + (pix / HW) * WP + pix % HW + 3;
  }
  const float* __restrict__ wrow = w_s + (h * 16 + n) * KP + kq * 9;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* __restrict__ a0 = in_s + abase[0];
  const float* __restrict__ a1 = in_s + abase[1];
  const float* __restrict__ a2 = in_s + abase[2];
  const float* __restrict__ a3 = in_s + abase[3];
  // the operands of k-step q + 1 are fetched from LDS while the matrix pipe works on k-step q (the compiler's own
  // schedule waited for every fetch right before its use)
  auto run = [&](auto four_c) {
    constexpr bool FOUR = decltype(four_c)::value;
    float bc, ac[4], bn = 0.f, an[4] = {0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int q, float& bv, float (&av)[4]) {
      const int tap = q / KSTEPS, kk = q % KSTEPS;
      bv = wrow[4 * kk * 9 + tap];
      const int off = 4 * kk * CS_F + (tap / 3) * WP + tap % 3;
      av[0] = a0[off]; av[1] = a1[off]; av[2] = a2[off];
      if (FOUR) av[3] = a3[off];
    };
    fetch(0, bc, ac);
#pragma unroll
    for (int q = 0; q < 9 * KSTEPS; ++q) {
      if (q + 1 < 9 * KSTEPS) fetch(q + 1, bn, an);
      __builtin_amdgcn_sched_barrier(0);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[0], bc, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[1], bc, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[2], bc, acc[2], 0, 0, 0);
      if (FOUR) acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[3], bc, acc[3], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      bc = bn; ac[0] = an[0]; ac[1] = an[1]; ac[2] = an[2]; ac[3] = an[3];
    }
  };
  if (four) run(std::true_type{}); else run(std::false_type{});
  CONV50_STAMP(2);
  // D[row = pixel 4 kq + j][col = channel n]: 4 consecutive pixels of the flattened plane per lane
  const int co = pair * WROWS + h * 16 + n;
  if constexpr (POOL_EPI) {
    // the workgroup's 32 planes go to LDS (over the image, which nobody reads any more), then one thread per window
    constexpr int YS = NPIX + 8;
    __syncthreads();
    float* __restrict__ y_s = lds;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = 16 * (t0 + 4 * j) + 4 * kq;
      if ((j < 3 || four) && p < NPIX)
        *reinterpret_cast<float4*>(y_s + (h * 16 + n) * YS + p) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    }
    __syncthreads();
    for (int i = tid; i < WROWS * PCELLS; i += T) {
      const int cl = i / PCELLS, cell = i % PCELLS, oi = cell / PH, oj = cell % PH, c = pair * WROWS + cl;
      if (c >= C) break;
      const float* __restrict__ src = y_s + cl * YS + 2 * oi * HW + 2 * oj;
      const float2 r0 = *reinterpret_cast<const float2*>(src);
      const float2 r1 = *reinterpret_cast<const float2*>(src + HW);
      const size_t o = ((size_t)img * C + c) * PCELLS + cell;
      int k;
      pa.pooled[o] = conv::pool_window(r0, r1, pa.bias ? pa.bias[c] : 0.f, &k);
      pa.code[o] = (uint8_t)k;
    }
  } else if (co < C) {
    float* __restrict__ yo = y + ((size_t)img * C + co) * NPIX;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = 16 * (t0 + 4 * j) + 4 * kq;
      if ((j < 3 || four) && p < NPIX) sgmcmc_store4<16>(y, yo + p, acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    }
  }
  CONV50_STAMP(3);
}


template <bool TRANSPOSE_W>
__global__ __launch_bounds__(T) void conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                   float* __restrict__ y, float* __restrict__ wT) {
  // (XCD-aware block order, as the trunk: an image's two workgroups and, across launches, its layers meet in one L2; round 6)
  conv_body<TRANSPOSE_W>(conv::xcd_remap((int)blockIdx.x, (int)gridDim.x), (int)gridDim.x, x, w, y, wT);
}
// forward with the tail
__global__ __launch_bounds__(T) void conv_pool_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      float* __restrict__ wT, PoolArgs pa) {
  conv_body<false, false, true>(conv::xcd_remap((int)blockIdx.x, (int)gridDim.x), (int)gridDim.x, x, w, nullptr, wT, pa);
}

// ---------------------------------------------------------------- weight gradient
// 8 waves: wave = (input-channel tile cit = w & 3, pixel half ps = w >> 2); the two halves' accumulators are added
// through LDS before the slab is written (fixed order: ps = 0 then ps = 1).
// FROM_POOLED: dy = the gradient of the pooled map, pa.src_code its bytes; pa.dbias_part (may be NULL) takes the sum of
// the workgroup's images' gradients per channel of its tile, cells in order, images in order.
template <bool FROM_POOLED = false>
__device__ __forceinline__ void wrw_body(int b, const float* __restrict__ x, const float* __restrict__ dy,
                                         float* __restrict__ part, int n_img,
                                         const PoolArgs pa = PoolArgs{nullptr, nullptr, nullptr, nullptr, nullptr}) {
  extern __shared__ float lds[];
  float* __restrict__ in_s = lds;
  float* __restrict__ dy_s = lds + CPW * CS_W;
  float* __restrict__ db_s = dy_s + 16 * DS + 2;            // FROM_POOLED: the tile's [16][49] gradients as they came
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = b % CT, pw = b / CT;
  const int cit = wave & 3, ps = wave >> 2;
  const int n = lane & 15, kq = lane >> 4;
  constexpr int NG = NPIX / 4, G0 = (NG + 1) / 2;           // 49 pixel groups: 25 + 24
  constexpr int ND = 16 * (NPIX / 2);                       // the dy tile: 16 channels x 98 float2
  f32x4 acc[9];
#pragma unroll
  for (int rs = 0; rs < 9; ++rs) acc[rs] = f32x4{0.f, 0.f, 0.f, 0.f};
  // round 3: the NEXT image's operands are loaded into registers while the matrix pipe works on the current one, and
  // the operands of pixel group g + 1 are fetched from LDS during the 9 MFMAs of group g (conv_hip.inc, same change)
  ImageStage<CS_W, CPW> im;
  constexpr int NDP = 16 * PCELLS;                          // FROM_POOLED: 16 channels x 49 cells (float + byte)
  float2 rd[FROM_POOLED ? 1 : (ND + T - 1) / T];
  float pd[FROM_POOLED ? (NDP + T - 1) / T : 1];
  uint8_t pk[FROM_POOLED ? (NDP + T - 1) / T : 1];
  float bsum = 0.f;
  auto load_item = [&](int img) {
    im.load(x + (size_t)img * C * NPIX);
    if constexpr (FROM_POOLED) {
#pragma unroll
      for (int it = 0; it < (NDP + T - 1) / T; ++it) {
        const int i = tid + it * T, co = ct * 16 + i / PCELLS;
        pd[it] = 0.f;
        pk[it] = 0;
        if (i < NDP && co < C) {
          pd[it] = dy[((size_t)img * C + co) * PCELLS + i % PCELLS];
          pk[it] = pa.src_code[((size_t)img * C + co) * PCELLS + i % PCELLS];
        }
      }
    } else {
      stage_load<ND, float2>(rd, [&](int i) {
        const int co = ct * 16 + i / (NPIX / 2);
        float2 q = make_float2(0.f, 0.f);
        if (co < C) q = *reinterpret_cast<const float2*>(dy + ((size_t)img * C + co) * NPIX + 2 * (i % (NPIX / 2)));
        return q;
      });
    }
  };
  if (pw * ITEMS < n_img) load_item(pw * ITEMS);
  ImageStage<CS_W, CPW>::zero_frame(in_s);                  // the frame and the padding plane stay zero
  // A = dy[co = n][pixel 4g + kq], B = x[ci = 16 cit + n][pixel + tap]
  const float* __restrict__ asrc = dy_s + n * DS + kq;
  const float* __restrict__ bsrc = in_s + min(cit * 16 + n, CPW - 1) * CS_W + 3;  // (columns >= 50 are discarded)
  const int g_begin = ps ? G0 : 0, n_g = ps ? NG - G0 : G0;
  for (int it = 0; it < ITEMS; ++it) {
    const int img = pw * ITEMS + it;
    if (img >= n_img) break;
    if (it) __syncthreads();                                // the previous image's operands are no longer being read
    im.store(in_s);
    if constexpr (FROM_POOLED) {
#pragma unroll
      for (int r = 0; r < (NDP + T - 1) / T; ++r) {
        const int i = tid + r * T;
        if (i < NDP) {
          const int cl = i / PCELLS, cell = i % PCELLS, oi = cell / PH, oj = cell % PH;
          db_s[i] = conv::unpool_window(dy_s + cl * DS + 2 * oi * HW + 2 * oj, HW, pd[r], pk[r]);
        }
      }
    } else {
      stage_store<ND, float2>(rd, [&](int i, const float2& q) {
        *reinterpret_cast<float2*>(dy_s + (i / (NPIX / 2)) * DS + 2 * (i % (NPIX / 2))) = q;
      });
    }
    __syncthreads();
    if (it + 1 < ITEMS && img + 1 < n_img) load_item(img + 1);
    if (FROM_POOLED && pa.dbias_part && tid < 16) {
#pragma unroll 7
      for (int cell = 0; cell < PCELLS; ++cell) bsum += db_s[tid * PCELLS + cell];
    }
    float a_cur, b_cur[9], a_nxt = 0.f, b_nxt[9];
    auto fetch = [&](int gi, float& a, float (&bv)[9]) {
      const int g = g_begin + gi;
      const int p = 4 * g + kq, row = p / HW, col = p - row * HW;
      a = asrc[4 * g];
      const float* __restrict__ bp = bsrc + row * WP + col;
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) bv[rs] = bp[(rs / 3) * WP + rs % 3];
    };
    fetch(0, a_cur, b_cur);
#pragma unroll
    for (int gi = 0; gi < G0; ++gi) {
      // (the second pixel half has one group less: its 25th step repeats the 24th group's fetch and skips the MFMAs)
      if (gi + 1 < G0) fetch(gi + 1 < n_g ? gi + 1 : gi, a_nxt, b_nxt);
      __builtin_amdgcn_sched_barrier(0);
      if (gi < n_g) {                                       // wave-uniform
#pragma unroll
        for (int rs = 0; rs < 9; ++rs) acc[rs] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur, b_cur[rs], acc[rs], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      a_cur = a_nxt;
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) b_cur[rs] = b_nxt[rs];
    }
  }
  if (FROM_POOLED && pa.dbias_part && tid < 16 && ct * 16 + tid < C) pa.dbias_part[(size_t)pw * C + ct * 16 + tid] = bsum;
  // add the two pixel halves through LDS, then the slab part[pw][co][ci][rs]: D[row = co 4 kq + j][col = ci n]
  __syncthreads();
  float* __restrict__ red = lds;                            // [cit][rs][64 lanes][4]
  if (ps == 1) {
#pragma unroll
    for (int rs = 0; rs < 9; ++rs)
      *reinterpret_cast<float4*>(red + ((cit * 9 + rs) * 64 + lane) * 4) =
          make_float4(acc[rs][0], acc[rs][1], acc[rs][2], acc[rs][3]);
  }
  __syncthreads();
  if (ps == 0) {
    float* __restrict__ out = part + (size_t)pw * (C * C * 9);
    const int ci = cit * 16 + n;
#pragma unroll
    for (int rs = 0; rs < 9; ++rs) {
      const float4 o = *reinterpret_cast<const float4*>(red + ((cit * 9 + rs) * 64 + lane) * 4);
      const float v[4] = {acc[rs][0] + o.x, acc[rs][1] + o.y, acc[rs][2] + o.z, acc[rs][3] + o.w};
      if (ci < C) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int co = ct * 16 + 4 * kq + j;
          if (co < C) out[((size_t)rs * C + co) * C + ci] = v[j];   // tap-major slab (conv_hip.inc)
        }
      }
    }
  }
}

__global__ __launch_bounds__(T, 1) void wrw_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                float* __restrict__ part, int n_img) {
  wrw_body(conv::xcd_remap((int)blockIdx.x, (int)gridDim.x), x, dy, part, n_img);
}

// both gradients in one launch; the weight-gradient workgroups (two images each: the long ones) first
__global__ __launch_bounds__(T, 1) void bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                const float* __restrict__ dy, float* __restrict__ dx,
                                                float* __restrict__ part, int n_wrw, int n_img) {
  const int b = (int)blockIdx.x;
  if (b < n_wrw) wrw_body(conv::xcd_remap(b, n_wrw), x, dy, part, n_img);
  else conv_body<true>(conv::xcd_remap(b - n_wrw, (int)gridDim.x - n_wrw), (int)gridDim.x - n_wrw, dy, w, dx);
}

// ... with the weights as the forward left them for the data gradient (wT): the forward's straight-copy staging
__global__ __launch_bounds__(T, 1) void bwd_t_kernel(const float* __restrict__ x, const float* __restrict__ wT,
                                                  const float* __restrict__ dy, float* __restrict__ dx,
                                                  float* __restrict__ part, int n_wrw, int n_img) {
  const int b = (int)blockIdx.x;
  if (b < n_wrw) wrw_body(conv::xcd_remap(b, n_wrw), x, dy, part, n_img);
  else conv_body<false>(conv::xcd_remap(b - n_wrw, (int)gridDim.x - n_wrw), (int)gridDim.x - n_wrw, dy, wT, dx);
}

// both gradients of the layer WITH its tail: dy = gradient of the pooled map + bytes; wT as bwd_t_kernel
__global__ __launch_bounds__(T, 1) void bwd_pool_kernel(const float* __restrict__ x, const float* __restrict__ wT,
                                                     const float* __restrict__ dpooled, float* __restrict__ dx,
                                                     float* __restrict__ part, int n_wrw, int n_img, PoolArgs pa) {
  const int b = (int)blockIdx.x;
  if (b < n_wrw) wrw_body<true>(conv::xcd_remap(b, n_wrw), x, dpooled, part, n_img, pa);
  else conv_body<false, true, false>(conv::xcd_remap(b - n_wrw, (int)gridDim.x - n_wrw), (int)gridDim.x - n_wrw, dpooled, wT, dx, nullptr, pa);
}

inline int prepare() {
  static bool done = false;
  if (done) return 0;
  const size_t both = LDS_FWD > LDS_W ? LDS_FWD : LDS_W;
  const struct { const void* k; size_t lds; } ks[] = {
      {reinterpret_cast<const void*>(conv_kernel<false>), LDS_FWD}, {reinterpret_cast<const void*>(conv_kernel<true>), LDS_FWD},
      {reinterpret_cast<const void*>(wrw_kernel), LDS_W}, {reinterpret_cast<const void*>(bwd_kernel), both},
      {reinterpret_cast<const void*>(bwd_t_kernel), both}, {reinterpret_cast<const void*>(bwd_pool_kernel), both},
      {reinterpret_cast<const void*>(conv_pool_kernel), LDS_FWD}};
  for (const auto& e : ks) {
    const hipError_t err = hipFuncSetAttribute(e.k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e.lds);
    if (err != hipSuccess) return (int)err;
  }
  done = true;
  return 0;
}

}  // namespace conv50

extern "C" int sgmcmc_conv50(const float* x, const float* w, float* y, int n_img, int transpose_w, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !y || n_img <= 0) return (int)hipErrorInvalidValue;
  if (const int e = conv50::prepare()) return e;
  const dim3 grid((unsigned)(n_img * conv50::NSUB)), block(conv50::T);
  float* none = nullptr;
  if (transpose_w) SGMCMC_LAUNCH(conv50::conv_kernel<true>, grid, block, conv50::LDS_FWD, (hipStream_t)stream, x, w, y, none);
  else SGMCMC_LAUNCH(conv50::conv_kernel<false>, grid, block, conv50::LDS_FWD, (hipStream_t)stream, x, w, y, none);
  return (int)hipGetLastError();
}

// forward that also leaves wT[ci][co][rs] = w[co][ci][8 - rs] (50*50*9 floats; may be NULL) for sgmcmc_conv50_bwd_t /
// for a data gradient through this same entry point (x = dy, w = wT)
extern "C" int sgmcmc_conv50_fwd(const float* x, const float* w, float* y, float* wT, int n_img, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !y || n_img <= 0) return (int)hipErrorInvalidValue;
  if (const int e = conv50::prepare()) return e;
  SGMCMC_LAUNCH(conv50::conv_kernel<false>, dim3((unsigned)(n_img * conv50::NSUB)), dim3(conv50::T), conv50::LDS_FWD,
                (hipStream_t)stream, x, w, y, wT);
  return (int)hipGetLastError();
}

extern "C" int64_t sgmcmc_conv50_scratch_floats(int n_img) {
  return n_img <= 0 ? -1 : (int64_t)((n_img + conv50::ITEMS - 1) / conv50::ITEMS) * conv50::C * conv50::C * 9;
}

extern "C" int sgmcmc_conv50_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* scratch,
                                 int n_img, int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !dy || !scratch || n_img <= 0 || (!dw && !deferred_slabs)) return (int)hipErrorInvalidValue;
  if (const int e = conv50::prepare()) return e;
  hipStream_t s = (hipStream_t)stream;
  const int P = (n_img + conv50::ITEMS - 1) / conv50::ITEMS, n_wrw = P * conv50::CT;
  if (dx) {
    const size_t lds = conv50::LDS_FWD > conv50::LDS_W ? conv50::LDS_FWD : conv50::LDS_W;
    SGMCMC_LAUNCH(conv50::bwd_kernel, dim3((unsigned)(n_wrw + n_img * conv50::NSUB)), dim3(conv50::T), lds, s, x, w, dy, dx,
                  scratch, n_wrw, n_img);
  } else {
    SGMCMC_LAUNCH(conv50::wrw_kernel, dim3((unsigned)n_wrw), dim3(conv50::T), conv50::LDS_W, s, x, dy, scratch, n_img);
  }
  return conv::finish_slabs(deferred_slabs, P, s, {{scratch, conv50::C * conv50::C * 9, dw, 9}});
}

// as sgmcmc_conv50_bwd with the data gradient's weights prepared by sgmcmc_conv50_fwd (wT): dx required
extern "C" int sgmcmc_conv50_bwd_t(const float* x, const float* wT, const float* dy, float* dx, float* dw, float* scratch,
                                   int n_img, int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !wT || !dy || !dx || !scratch || n_img <= 0 || (!dw && !deferred_slabs)) return (int)hipErrorInvalidValue;
  if (const int e = conv50::prepare()) return e;
  hipStream_t s = (hipStream_t)stream;
  const int P = (n_img + conv50::ITEMS - 1) / conv50::ITEMS, n_wrw = P * conv50::CT;
  const size_t lds = conv50::LDS_FWD > conv50::LDS_W ? conv50::LDS_FWD : conv50::LDS_W;
  SGMCMC_LAUNCH(conv50::bwd_t_kernel, dim3((unsigned)(n_wrw + n_img * conv50::NSUB)), dim3(conv50::T), lds, s, x, wT, dy, dx,
                scratch, n_wrw, n_img);
  return conv::finish_slabs(deferred_slabs, P, s, {{scratch, conv50::C * conv50::C * 9, dw, 9}});
}

/* the layer WITH its tail, Conv2d(50, 50, 3, padding=1) -> + bias -> ReLU -> MaxPool2d(2): pooled [n][50][7][7],
 * code [n][50][7][7] bytes (sgmcmc_conv_first_pool_fwd's encoding), wT as sgmcmc_conv50_fwd (may be NULL) */
extern "C" int sgmcmc_conv50_pool_fwd(const float* x, const float* w, const float* bias, float* pooled, uint8_t* code,
                                      float* wT, int n_img, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !pooled || !code || n_img <= 0) return (int)hipErrorInvalidValue;
  if (const int e = conv50::prepare()) return e;
  const conv50::PoolArgs pa = {bias, pooled, code, nullptr, nullptr};
  SGMCMC_LAUNCH(conv50::conv_pool_kernel, dim3((unsigned)(n_img * conv50::NSUB)), dim3(conv50::T), conv50::LDS_FWD,
                (hipStream_t)stream, x, w, wT, pa);
  return (int)hipGetLastError();
}

extern "C" int64_t sgmcmc_conv50_pool_scratch_floats(int n_img) {
  return n_img <= 0 ? -1 : (int64_t)((n_img + conv50::ITEMS - 1) / conv50::ITEMS) * (conv50::C * conv50::C * 9 + conv50::C);
}

/* its backward from the gradient w.r.t. pooled (+ code): dx [n][50][14][14], weight-gradient slabs [P][22500] at
 * scratch and, with want_bias, bias-gradient slabs [P][50] behind them (P = ceil(n_img / 2)); dw / dbias reduced here
 * or -- deferred_slabs != NULL -- left to the caller's sgmcmc_wrw_reduce_many (weight slabs tap-major: taps = 9) */
extern "C" int sgmcmc_conv50_pool_bwd(const float* x, const float* wT, const float* dpooled, const uint8_t* code, float* dx,
                                      float* dw, float* dbias, float* scratch, int n_img, int want_bias,
                                      int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !wT || !dpooled || !code || !dx || !scratch || n_img <= 0 || (!deferred_slabs && (!dw || (want_bias && !dbias))))
    return (int)hipErrorInvalidValue;
  if (const int e = conv50::prepare()) return e;
  hipStream_t s = (hipStream_t)stream;
  const int P = (n_img + conv50::ITEMS - 1) / conv50::ITEMS, n_wrw = P * conv50::CT, E = conv50::C * conv50::C * 9;
  float* bpart = want_bias ? scratch + (size_t)P * E : nullptr;
  const size_t lds = conv50::LDS_FWD > conv50::LDS_W ? conv50::LDS_FWD : conv50::LDS_W;
  const conv50::PoolArgs pa = {nullptr, nullptr, nullptr, code, bpart};
  SGMCMC_LAUNCH(conv50::bwd_pool_kernel, dim3((unsigned)(n_wrw + n_img * conv50::NSUB)), dim3(conv50::T), lds, s, x, wT,
                dpooled, dx, scratch, n_wrw, n_img, pa);
  return conv::finish_slabs(deferred_slabs, P, s,
                            {{scratch, E, dw, 9}, {bpart, conv50::C, want_bias ? dbias : nullptr, 1}});
}
