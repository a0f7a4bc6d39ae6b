// The two convolutions that open a down-sampling ResNet block (models/google_resnet.py:77-90), as ONE
// operator: the 3x3 / stride 2 / pad 1 convolution of the main path and the 1x1 / stride 2 shortcut read
// the same input, and the shortcut's operand x[n,ci,2oy,2ox] is exactly the 3x3's centre tap -- so the
// shortcut rides along as a tenth "tap" with its own weights, accumulators and output.
//
//   ym[n,co,oy,ox] = sum_{ci,r,s} x[n,ci,2oy+r-1,2ox+s-1] wm[co,ci,r,s]        ys[n,co,oy,ox] = sum_ci x[n,ci,2oy,2ox] ws[co,ci]
//   dx[n,ci,iy,ix] = sum_{co,(r,s): iy=2oy+r-1, ix=2ox+s-1} dym[n,co,oy,ox] wm[co,ci,r,s]  (+ sum_co dys ws at even iy, ix)
//   dwm[co,ci,r,s] = sum_{n,o} dym[n,co,o] x[n,ci,2o+(r-1,s-1)]                  dws[co,ci] = sum_{n,o} dys[n,co,o] x[n,ci,2o]
//
// CIN -> COUT = 2 CIN channels, HWI -> HWO = HWI / 2 pixels: (16, 32) and (32, 16).  Same machinery as
// conv_hip.inc: fp32 MFMA 16x16x4, operands staged in LDS, 512 workgroups of 4 waves per launch (256 for
// the weight gradient), per-band batch statistics from the accumulators, weight-gradient slabs reduced
// in a fixed order.

namespace convdown {

using f32x4 = __attribute__((ext_vector_type(4))) float;

template <int CIN, int HWI>
struct Cfg {
  static constexpr int COUT = 2 * CIN, HWO = HWI / 2;
  static constexpr int ROWS_O = 8;                     // output rows per band
  static constexpr int ROWS_I = 2 * ROWS_O + 1;        // input rows iy = 2*oy0 - 1 .. 2*oy0 + 15
  static constexpr int WP = HWI + 8;                   // 4 pad | W | 4 pad, halo at 3 and W + 4
  static constexpr int CS_RAW = ROWS_I * WP;
  static constexpr int CS = CS_RAW + ((16 - CS_RAW % 64) % 64 + 64) % 64 % 64;  // = 16 mod 64
  static constexpr int K = 9 * CIN, KP = K + ((2 - K % 32) % 32 + 32) % 32, KSP = CIN + 1;   // (pitch = 2 mod 32: conv_hip.inc)
  static constexpr int BANDS = HWO / ROWS_O, CT = COUT / 16;
  static constexpr int PT = ROWS_O * HWO / 16, PT_W = PT / 4;
  static constexpr size_t LDS_BYTES = (size_t)(CIN * CS + 16 * KP + 16 * KSP) * sizeof(float);
  static_assert(PT % 4 == 0 && PT_W >= 1, "4 waves share the pixel tiles");
};

// input band with halo; CS: channel stride of the destination (forward and wrw differ).  Split into a load
// phase and a store phase (conv::stage_load / stage_store) so that callers keep ALL their operands' global
// loads in flight before the first LDS store.
template <int CIN, int HWI>
struct InputStage {
  static constexpr int V = HWI / 4, ROWS_I = Cfg<CIN, HWI>::ROWS_I, WP = Cfg<CIN, HWI>::WP;
  static constexpr int TOTAL = CIN * ROWS_I * V, IT = (TOTAL + 255) / 256;
  float4 r[IT];
  __device__ __forceinline__ void load(const float* __restrict__ xi, int iy0) {
    conv::stage_load<TOTAL, float4>(r, [&](int i) {
      const int v = i % V, ry = (i / V) % ROWS_I, ci = i / (V * ROWS_I);
      const int gy = iy0 + ry;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gy >= 0 && gy < HWI) val = *reinterpret_cast<const float4*>(xi + ((size_t)ci * HWI + gy) * HWI + 4 * v);
      return val;
    });
  }
  template <int CS>
  __device__ __forceinline__ void store(float* __restrict__ in_s, int tid) const {
    conv::stage_store<TOTAL, float4>(r, [&](int i, const float4& val) {
      const int v = i % V, ry = (i / V) % ROWS_I, ci = i / (V * ROWS_I);
      *reinterpret_cast<float4*>(in_s + ci * CS + ry * WP + 4 + 4 * v) = val;
    });
    for (int i = tid; i < CIN * ROWS_I * 2; i += 256) {
      const int side = i & 1, ry = (i >> 1) % ROWS_I, ci = (i >> 1) / ROWS_I;
      in_s[ci * CS + ry * WP + (side ? HWI + 4 : 3)] = 0.f;
    }
  }
};

// ---------------------------------------------------------------- forward
template <int CIN, int HWI, bool STATS>
__global__ __launch_bounds__(256) void fwd_kernel(const float* __restrict__ x, const float* __restrict__ wm,
                                                  const float* __restrict__ ws, float* __restrict__ ym,
                                                  float* __restrict__ ys, double* __restrict__ stats_m,
                                                  double* __restrict__ stats_s, int n_slices) {
  using G = Cfg<CIN, HWI>;
  constexpr int HWO = G::HWO, COUT = G::COUT;
  extern __shared__ float lds[];
  float* __restrict__ in_s = lds;
  float* __restrict__ w_s = lds + CIN * G::CS;
  float* __restrict__ ws_s = w_s + 16 * G::KP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (XCD-aware block order, as the trunk's kernels: an image's bands and channel tiles meet in one L2; round 6)
  int b = conv::xcd_remap<CIN>((int)blockIdx.x, (int)gridDim.x);
  const int ct = b % G::CT;
  b /= G::CT;
  const int band = b % G::BANDS, img = b / G::BANDS;
  const int oy0 = band * G::ROWS_O;

  {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(wm + (size_t)ct * 16 * G::K);
    const float* __restrict__ ssrc = ws + (size_t)ct * 16 * CIN;
    float4 rw[(4 * G::K + 255) / 256];
    float rs_[(16 * CIN + 255) / 256];
    InputStage<CIN, HWI> in;
    conv::stage_load<4 * G::K, float4>(rw, [&](int i) { return src[i]; });
    conv::stage_load<16 * CIN, float>(rs_, [&](int i) { return ssrc[i]; });
    in.load(x + (size_t)img * CIN * HWI * HWI, 2 * oy0 - 1);
    conv::stage_store<4 * G::K, float4>(rw, [&](int i, const float4& q) {
      float* d = w_s + (4 * i / G::K) * G::KP + (4 * i) % G::K;
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    });
    conv::stage_store<16 * CIN, float>(rs_, [&](int i, float q) { ws_s[(i / CIN) * G::KSP + i % CIN] = q; });
    in.template store<G::CS>(in_s, tid);
  }
  __syncthreads();

  const int n = lane & 15, kq = lane >> 4;
  constexpr int NACC = G::PT_W == 1 ? 2 : G::PT_W;
  f32x4 acc[NACC], accs[G::PT_W];
  int abase[G::PT_W], orow[G::PT_W], ocol[G::PT_W];
#pragma unroll
  for (int t = 0; t < G::PT_W; ++t) {
    const int p = wave * G::PT_W + t;
    int oy, ox;
    if (HWO >= 16) { oy = p; ox = n; }                  // a tile = one output row of 16 pixels
    else { oy = 2 * p + (n >> 3); ox = n & 7; }         // or two rows of 8
    abase[t] = kq * G::CS + (2 * oy) * G::WP + 2 * ox + 3;
    const int m0 = 4 * kq;
    if (HWO >= 16) { orow[t] = p; ocol[t] = m0; }
    else { orow[t] = 2 * p + (m0 >> 3); ocol[t] = m0 & 7; }
    accs[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int a = 0; a < NACC; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int rs = 0; rs < 9; ++rs) {
    const int r = rs / 3, s = rs % 3;
#pragma unroll
    for (int kk = 0; kk < CIN / 4; ++kk) {
      const float bv = w_s[n * G::KP + (4 * kk + kq) * 9 + rs];
      const float bs = rs == 4 ? ws_s[n * G::KSP + 4 * kk + kq] : 0.f;
#pragma unroll
      for (int t = 0; t < G::PT_W; ++t) {
        const float a = in_s[abase[t] + 4 * kk * G::CS + r * G::WP + s];
        const int ai = G::PT_W == 1 ? (kk & 1) : t;
        acc[ai] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[ai], 0, 0, 0);
        if (rs == 4) accs[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs, accs[t], 0, 0, 0);
      }
    }
  }
  const size_t obase = ((size_t)img * COUT + ct * 16 + n) * HWO * HWO;
  f32x4 vm[G::PT_W], vs[G::PT_W];
  float m1 = 0.f, q1 = 0.f;
#pragma unroll
  for (int t = 0; t < G::PT_W; ++t) {
    f32x4 v = acc[t];
    if (G::PT_W == 1) v += acc[1];
    const f32x4 u = accs[t];
    vm[t] = v;
    vs[t] = u;
    const size_t o = obase + (size_t)(oy0 + orow[t]) * HWO + ocol[t];
    sgmcmc_store4<4>(ym, ym + o, v[0], v[1], v[2], v[3]);
    sgmcmc_store4<4>(ys, ys + o, u[0], u[1], u[2], u[3]);
    if (STATS) {
      m1 += (v[0] + v[1]) + (v[2] + v[3]);
      q1 += (u[0] + u[1]) + (u[2] + u[3]);
    }
  }
  if (STATS) {
    const size_t so = ((size_t)(ct * 16) * n_slices + (img * G::BANDS + band)) * 2;
    conv::band_stats<G::PT_W>(vm, m1, G::ROWS_O * HWO, lds, stats_m + so, (size_t)n_slices * 2);
    conv::band_stats<G::PT_W>(vs, q1, G::ROWS_O * HWO, lds, stats_s + so, (size_t)n_slices * 2);
  }
}

template <int CIN, int HWI>
int launch_fwd(const float* x, const float* wm, const float* ws, float* ym, float* ys, double* stats_m,
               double* stats_s, int n_img, hipStream_t s) {
  using G = Cfg<CIN, HWI>;
  auto k0 = fwd_kernel<CIN, HWI, false>;
  auto k1 = fwd_kernel<CIN, HWI, true>;
  static bool attr_done = false;
  if (!attr_done) {
    for (const void* k : {reinterpret_cast<const void*>(k0), reinterpret_cast<const void*>(k1)}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  const dim3 grid((unsigned)(n_img * G::BANDS * G::CT)), block(256);
  const int n_slices = n_img * G::BANDS;
  if (stats_m) SGMCMC_LAUNCH(k1, grid, block, G::LDS_BYTES, s, x, wm, ws, ym, ys, stats_m, stats_s, n_slices);
  else SGMCMC_LAUNCH(k0, grid, block, G::LDS_BYTES, s, x, wm, ws, ym, ys, nullptr, nullptr, n_slices);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- data gradient
// dx by parity class of the input pixel (iy & 1, ix & 1): only the taps with iy = 2 oy + r - 1 and
// ix = 2 ox + s - 1 contribute -- 1 tap for (even, even) (plus the shortcut), 2 for the mixed classes, 4 for
// (odd, odd) -- so no multiply is spent on the zeros of a dilated gradient.  A pixel tile = 16 pixels of
// ONE class: j = 0..15 along a row (32-pixel images) or 8 + 8 over two rows of equal parity (16-pixel).
template <int CIN, int HWI>
struct DCfg {
  static constexpr int COUT = 2 * CIN, HWO = HWI / 2;
  static constexpr int ROWS_I = 8, ROWS_O = ROWS_I / 2 + 1;  // 8 input rows need output rows a0 .. a0 + 4
  static constexpr int WPO = HWO + 8;
  static constexpr int DS_RAW = ROWS_O * WPO;
  static constexpr int DS = DS_RAW + ((16 - DS_RAW % 64) % 64 + 64) % 64;  // = 16 mod 64 (k-lanes = channels)
  static constexpr int K = 9 * COUT, KP = K + ((2 - K % 32) % 32 + 32) % 32, KSP = COUT + 1;
  static constexpr int BANDS = HWI / ROWS_I, CT = CIN / 16;
  static constexpr size_t LDS_BYTES = (size_t)(2 * COUT * DS + 16 * KP + 16 * KSP) * sizeof(float);
};

template <int CIN, int HWI, int PY, int PX>
__device__ __forceinline__ f32x4 dgrad_tile(const float* __restrict__ dym_s, const float* __restrict__ dys_s,
                                             const float* __restrict__ w_s, const float* __restrict__ ws_s,
                                             int abase, int n, int kq) {
  using G = DCfg<CIN, HWI>;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = (PY ? 0 : 1); r < 3; r += 2) {
    const int oy_off = (PY && r == 0) ? 1 : 0;     // odd iy: r = 0 reaches the output row below
#pragma unroll
    for (int s = (PX ? 0 : 1); s < 3; s += 2) {
      const int ox_off = (PX && s == 0) ? 1 : 0;
      const int rs = r * 3 + s;
#pragma unroll
      for (int kk = 0; kk < G::COUT / 4; ++kk) {
        const float a = dym_s[abase + 4 * kk * G::DS + oy_off * G::WPO + ox_off];
        const float bv = w_s[n * G::KP + (4 * kk + kq) * 9 + rs];
        if (kk & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc1, 0, 0, 0);
        else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc0, 0, 0, 0);
      }
    }
  }
  if (PY == 0 && PX == 0) {
#pragma unroll
    for (int kk = 0; kk < G::COUT / 4; ++kk) {
      const float a = dys_s[abase + 4 * kk * G::DS];
      const float bv = ws_s[n * G::KSP + 4 * kk + kq];
      if (kk & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc1, 0, 0, 0);
      else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc0, 0, 0, 0);
    }
  }
  return acc0 + acc1;
}

// SUMS: as conv3x3_body's (conv_hip.inc) -- the partial sums of the BatchNorm backward whose incoming gradient dx is.
template <int CIN, int HWI, bool SUMS>
__device__ __forceinline__ void dgrad_body(int b, const float* __restrict__ wm, const float* __restrict__ ws,
                                           const float* __restrict__ dym, const float* __restrict__ dys,
                                           float* __restrict__ dx, const conv::BwdEpilogue* E) {
  using G = DCfg<CIN, HWI>;
  constexpr int COUT = G::COUT, HWO = G::HWO;
  extern __shared__ float lds[];
  float* __restrict__ dym_s = lds;
  float* __restrict__ dys_s = lds + COUT * G::DS;
  float* __restrict__ w_s = dys_s + COUT * G::DS;
  float* __restrict__ ws_s = w_s + 16 * G::KP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = b % G::CT;
  b /= G::CT;
  const int band = b % G::BANDS, img = b / G::BANDS;
  const int iy0 = band * G::ROWS_I, a0 = iy0 / 2;

  // weights of this input-channel tile: w_s[n = ci][(co, r, s)] = wm[co][ct*16 + n][r][s]; ws_s[n][co];
  // the two output-gradient bands, rows a0 .. a0 + 4 (zero beyond the image), right halo column zero --
  // every global load in flight before the first LDS store
  {
    constexpr int V = HWO / 4, NB = 2 * COUT * G::ROWS_O * V;
    const size_t ibase = (size_t)img * COUT * HWO * HWO;
    float rw[(16 * G::K + 255) / 256];
    float rs_[(16 * COUT + 255) / 256];
    float4 rb[(NB + 255) / 256];
    conv::stage_load<16 * G::K, float>(rw, [&](int i) {
      const int n = i / G::K, kidx = i % G::K, co = kidx / 9, rs = kidx % 9;
      return wm[((size_t)co * CIN + (ct * 16 + n)) * 9 + rs];
    });
    conv::stage_load<16 * COUT, float>(rs_, [&](int i) {
      const int n = i / COUT, co = i % COUT;
      return ws[(size_t)co * CIN + ct * 16 + n];
    });
    conv::stage_load<NB, float4>(rb, [&](int i) {
      const int v = i % V, ry = (i / V) % G::ROWS_O, c2 = i / (V * G::ROWS_O);
      const int which = c2 / COUT, co = c2 % COUT, gy = a0 + ry;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gy < HWO)
        val = *reinterpret_cast<const float4*>((which ? dys : dym) + ibase + ((size_t)co * HWO + gy) * HWO + 4 * v);
      return val;
    });
    conv::stage_store<16 * G::K, float>(rw, [&](int i, float q) { w_s[(i / G::K) * G::KP + i % G::K] = q; });
    conv::stage_store<16 * COUT, float>(rs_, [&](int i, float q) { ws_s[(i / COUT) * G::KSP + i % COUT] = q; });
    conv::stage_store<NB, float4>(rb, [&](int i, const float4& val) {
      const int v = i % V, ry = (i / V) % G::ROWS_O, c2 = i / (V * G::ROWS_O);
      const int which = c2 / COUT, co = c2 % COUT;
      *reinterpret_cast<float4*>((which ? dys_s : dym_s) + co * G::DS + ry * G::WPO + 4 + 4 * v) = val;
    });
    for (int i = tid; i < 2 * COUT * G::ROWS_O; i += 256) {
      const int ry = i % G::ROWS_O, c2 = i / G::ROWS_O;
      ((c2 / COUT) ? dys_s : dym_s)[(c2 % COUT) * G::DS + ry * G::WPO + HWO + 4] = 0.f;
    }
  }
  __syncthreads();

  const int n = lane & 15, kq = lane >> 4;
  float* __restrict__ dxo = dx + ((size_t)img * CIN + ct * 16 + n) * HWI * HWI;
  float z1 = 0.f, z2 = 0.f, s_mean = 0.f, s_invstd = 0.f;
  if (SUMS) {
    const int go = conv::group_offset(E, img, CIN);
    s_mean = E->s_mean[go + ct * 16 + n]; s_invstd = E->s_invstd[go + ct * 16 + n];
  }
  // one float4 of dx stored at `dst`, and (SUMS) its share of sum dz, sum dz * xhat (o, q: the mask / BatchNorm input
  // there, loaded BEFORE the MFMA phase so that their latency hides under it); with E->mask_dx what is stored is dz
  const bool mask_dx = SUMS && E->mask_dx;
  auto put4 = [&](float* dst, const float4& o, const float4& q, float v0, float v1, float v2, float v3) {
    if (SUMS) {
      const float d0 = o.x > 0.f ? v0 : 0.f, d1 = o.y > 0.f ? v1 : 0.f, d2 = o.z > 0.f ? v2 : 0.f, d3 = o.w > 0.f ? v3 : 0.f;
      z1 += (d0 + d1) + (d2 + d3);
      z2 += (d0 * ((q.x - s_mean) * s_invstd) + d1 * ((q.y - s_mean) * s_invstd)) +
            (d2 * ((q.z - s_mean) * s_invstd) + d3 * ((q.w - s_mean) * s_invstd));
      if (mask_dx) { v0 = d0; v1 = d1; v2 = d2; v3 = d3; }
    }
    *reinterpret_cast<float4*>(dst) = make_float4(v0, v1, v2, v3);   // (write-through measured +1 us here at 16 -> 32 channels: plain)
  };
  if (HWI >= 32) {
    // wave w: input rows iy0 + 2w (even) and iy0 + 2w + 1 (odd); lane row m = j, pixels ix = 2j + px
    const int abase = kq * G::DS + wave * G::WPO + n + 4;
    float* re = dxo + (size_t)(iy0 + 2 * wave) * HWI + 8 * kq;   // j = 4kq .. 4kq+3 -> ix = 8kq .. 8kq+7
    float4 so[4] = {}, sq[4] = {};
    if (SUMS) {
      const size_t off = (size_t)(re - dx);
      const size_t offs[4] = {off, off + 4, off + HWI, off + HWI + 4};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        so[i] = *reinterpret_cast<const float4*>(E->s_out + offs[i]);
        sq[i] = *reinterpret_cast<const float4*>(E->s_y + offs[i]);
      }
    }
    const f32x4 e0 = dgrad_tile<CIN, HWI, 0, 0>(dym_s, dys_s, w_s, ws_s, abase, n, kq);
    const f32x4 e1 = dgrad_tile<CIN, HWI, 0, 1>(dym_s, dys_s, w_s, ws_s, abase, n, kq);
    const f32x4 o0 = dgrad_tile<CIN, HWI, 1, 0>(dym_s, dys_s, w_s, ws_s, abase, n, kq);
    const f32x4 o1 = dgrad_tile<CIN, HWI, 1, 1>(dym_s, dys_s, w_s, ws_s, abase, n, kq);
    put4(re, so[0], sq[0], e0[0], e1[0], e0[1], e1[1]);
    put4(re + 4, so[1], sq[1], e0[2], e1[2], e0[3], e1[3]);
    put4(re + HWI, so[2], sq[2], o0[0], o1[0], o0[1], o1[1]);
    put4(re + HWI + 4, so[3], sq[3], o0[2], o1[2], o0[3], o1[3]);
  } else {
    // wave w: parity py = w >> 1, row pair q = w & 1: rows iy0 + 4q + py and + 2; lane row m = (rowsel, j)
    const int py = wave >> 1, q = wave & 1;
    const int abase = kq * G::DS + (2 * q + (n >> 3)) * G::WPO + (n & 7) + 4;
    // D rows 4kq .. 4kq+3: rowsel = kq >> 1, j = 4 (kq & 1) .. + 3 -> ix = 8 (kq & 1) .. + 7
    float* re = dxo + (size_t)(iy0 + 4 * q + py + 2 * (kq >> 1)) * HWI + 8 * (kq & 1);
    float4 so[2] = {}, sq[2] = {};
    if (SUMS) {
      const size_t off = (size_t)(re - dx);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        so[i] = *reinterpret_cast<const float4*>(E->s_out + off + 4 * i);
        sq[i] = *reinterpret_cast<const float4*>(E->s_y + off + 4 * i);
      }
    }
    f32x4 t0, t1;
    if (py == 0) {
      t0 = dgrad_tile<CIN, HWI, 0, 0>(dym_s, dys_s, w_s, ws_s, abase, n, kq);
      t1 = dgrad_tile<CIN, HWI, 0, 1>(dym_s, dys_s, w_s, ws_s, abase, n, kq);
    } else {
      t0 = dgrad_tile<CIN, HWI, 1, 0>(dym_s, dys_s, w_s, ws_s, abase, n, kq);
      t1 = dgrad_tile<CIN, HWI, 1, 1>(dym_s, dys_s, w_s, ws_s, abase, n, kq);
    }
    put4(re, so[0], sq[0], t0[0], t1[0], t0[1], t1[1]);
    put4(re + 4, so[1], sq[1], t0[2], t1[2], t0[3], t1[3]);
  }
  if (SUMS) conv::band_sums(z1, z2, lds, E->s_partial + ((size_t)(ct * 16) * E->n_slices + (img * G::BANDS + band)) * 2,
                            (size_t)E->n_slices * 2);
}

// ---------------------------------------------------------------- weight gradients
template <int CIN, int HWI>
struct WCfg {
  static constexpr int COUT = 2 * CIN, HWO = HWI / 2;
  static constexpr int ROWS_O = 8, ROWS_I = 2 * ROWS_O + 1;
  static constexpr int WP = HWI + 8;
  static constexpr int CS_RAW = ROWS_I * WP;
  static constexpr int CS = CS_RAW + ((8 - CS_RAW % 64) % 64 + 64) % 64;  // n-lanes = channels, k-lanes 2 apart
  static constexpr int NPIX = ROWS_O * HWO, DS = NPIX + 4;
  static constexpr int NCI = CIN / 16, PS = 4 / NCI, KSTEPS = NPIX / 4 / PS;
  static constexpr int BANDS = HWO / ROWS_O, CT = COUT / 16, ITEMS = 2;
  static constexpr int E_MAIN = COUT * CIN * 9, E_SHORT = COUT * CIN;
  static constexpr size_t STAGE = (size_t)CIN * CS + 32 * DS, RED = 4 * 10 * 256;
  static constexpr size_t LDS_BYTES = (STAGE > RED ? STAGE : RED) * sizeof(float);
};

template <int CIN, int HWI>
__device__ __forceinline__ void wrw_body(int b, const float* __restrict__ x, const float* __restrict__ dym,
                                         const float* __restrict__ dys, float* __restrict__ part_m,
                                         float* __restrict__ part_s, int n_items) {
  using G = WCfg<CIN, HWI>;
  constexpr int COUT = G::COUT, HWO = G::HWO;
  extern __shared__ float lds[];
  float* __restrict__ in_s = lds;
  float* __restrict__ dm_s = lds + CIN * G::CS;
  float* __restrict__ dsh_s = dm_s + 16 * G::DS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = b % G::CT, pw = b / G::CT;
  const int cit = wave % G::NCI, ps = wave / G::NCI;
  const int n = lane & 15, kq = lane >> 4;
  f32x4 acc[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int it = 0; it < G::ITEMS; ++it) {
    const int item = pw * G::ITEMS + it;
    if (item >= n_items) break;
    const int band = item % G::BANDS, img = item / G::BANDS;
    const int oy0 = band * G::ROWS_O;
    if (it) __syncthreads();
    {
      constexpr int ND = 2 * 16 * G::NPIX / 4;
      const size_t dbase = (((size_t)img * COUT + ct * 16) * HWO + oy0) * HWO;
      InputStage<CIN, HWI> in;   // same WP, ROWS_I as the forward
      float4 rd[(ND + 255) / 256];
      in.load(x + (size_t)img * CIN * HWI * HWI, 2 * oy0 - 1);
      conv::stage_load<ND, float4>(rd, [&](int i) {
        const int v = i % (G::NPIX / 4), c2 = i / (G::NPIX / 4), which = c2 / 16, co = c2 % 16;
        return *reinterpret_cast<const float4*>((which ? dys : dym) + dbase + (size_t)co * HWO * HWO + 4 * v);
      });
      in.template store<G::CS>(in_s, tid);
      conv::stage_store<ND, float4>(rd, [&](int i, const float4& val) {
        const int v = i % (G::NPIX / 4), c2 = i / (G::NPIX / 4), which = c2 / 16, co = c2 % 16;
        *reinterpret_cast<float4*>((which ? dsh_s : dm_s) + co * G::DS + 4 * v) = val;
      });
    }
    __syncthreads();
    const float* __restrict__ bsrc = in_s + (cit * 16 + n) * G::CS + 2 * kq + 3;
#pragma unroll
    for (int kk = 0; kk < G::KSTEPS; ++kk) {
      const int g = ps * G::KSTEPS + kk;
      const int row = g / (HWO / 4), xg = g % (HWO / 4);
      const float am = dm_s[n * G::DS + 4 * g + kq], as = dsh_s[n * G::DS + 4 * g + kq];
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) {
        const float bv = bsrc[(2 * row + rs / 3) * G::WP + 8 * xg + rs % 3];
        acc[rs] = __builtin_amdgcn_mfma_f32_16x16x4f32(am, bv, acc[rs], 0, 0, 0);
        if (rs == 4) acc[9] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bv, acc[9], 0, 0, 0);
      }
    }
  }
  __syncthreads();
  float* __restrict__ red = lds;  // [wave][10][256]
#pragma unroll
  for (int i = 0; i < 10; ++i)
    *reinterpret_cast<float4*>(red + (wave * 10 + i) * 256 + 4 * lane) =
        make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
  __syncthreads();
  float* __restrict__ om = part_m + (size_t)pw * G::E_MAIN + (size_t)ct * 16 * CIN;   // tap-major slab (conv_hip.inc)
  float* __restrict__ os = part_s + (size_t)pw * G::E_SHORT + (size_t)ct * 16 * CIN;
  for (int i = tid; i < G::NCI * 10 * 256; i += 256) {
    const int e = i % 256, rs = (i / 256) % 10, ci_t = i / (256 * 10);
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < G::PS; ++q) v += red[((q * G::NCI + ci_t) * 10 + rs) * 256 + e];
    const int ln = e >> 2, vv = e & 3;
    const int co = 4 * (ln >> 4) + vv, ci = ci_t * 16 + (ln & 15);
    if (rs < 9) om[((size_t)rs * (2 * CIN) + co) * CIN + ci] = v;
    else os[(size_t)co * CIN + ci] = v;
  }
}

// data gradient and both weight gradients in one launch
template <int CIN, int HWI, bool SUMS>
__global__ __launch_bounds__(256) void bwd_kernel(const float* __restrict__ x, const float* __restrict__ wm,
                                                  const float* __restrict__ ws, const float* __restrict__ dym,
                                                  const float* __restrict__ dys, float* __restrict__ dx,
                                                  float* __restrict__ part_m, float* __restrict__ part_s,
                                                  int n_dgrad, int n_items, conv::BwdEpilogue E) {
  const int b = (int)blockIdx.x;
  const int n_wrw = (int)gridDim.x - n_dgrad;   // weight-gradient blocks (the long ones) first: see conv3x3_bwd_kernel
  if (b < n_wrw) wrw_body<CIN, HWI>(conv::xcd_remap<CIN>(b, n_wrw), x, dym, dys, part_m, part_s, n_items);
  else dgrad_body<CIN, HWI, SUMS>(conv::xcd_remap<CIN>(b - n_wrw, n_dgrad), wm, ws, dym, dys, dx, &E);
}

template <int CIN, int HWI>
int launch_bwd(const float* x, const float* wm, const float* ws, const float* dym, const float* dys, float* dx,
               float* dwm, float* dws, float* scratch, int n_img, int* n_slabs, hipStream_t s,
               const conv::BwdEpilogue& E = conv::BwdEpilogue{}) {
  using D = DCfg<CIN, HWI>;
  using W = WCfg<CIN, HWI>;
  const int n_items = n_img * W::BANDS, P = (n_items + W::ITEMS - 1) / W::ITEMS;
  const int n_dgrad = n_img * D::BANDS * D::CT;
  const size_t lds = D::LDS_BYTES > W::LDS_BYTES ? D::LDS_BYTES : W::LDS_BYTES;
  auto k = bwd_kernel<CIN, HWI, false>;
  auto ks = bwd_kernel<CIN, HWI, true>;
  static bool attr_done = false;
  if (!attr_done) {
    for (const void* f : {reinterpret_cast<const void*>(k), reinterpret_cast<const void*>(ks)}) {
      const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  float* part_m = scratch;
  float* part_s = scratch + (size_t)P * W::E_MAIN;
  conv::BwdEpilogue Ev = E;
  Ev.n_slices = n_img * D::BANDS;
  if (E.s_partial) SGMCMC_LAUNCH(ks, dim3((unsigned)(n_dgrad + P * W::CT)), dim3(256), lds, s, x, wm, ws, dym, dys, dx,
                                 part_m, part_s, n_dgrad, n_items, Ev);
  else SGMCMC_LAUNCH(k, dim3((unsigned)(n_dgrad + P * W::CT)), dim3(256), lds, s, x, wm, ws, dym, dys, dx, part_m,
                     part_s, n_dgrad, n_items, Ev);
  return conv::finish_slabs(n_slabs, P, s, {{part_m, W::E_MAIN, dwm, 9}, {part_s, W::E_SHORT, dws, 1}});
}

}  // namespace convdown

extern "C" int64_t sgmcmc_conv_down_scratch_floats(int n_img, int cin, int hwi) {
  if (!((cin == 16 && hwi == 32) || (cin == 32 && hwi == 16)) || n_img <= 0) return -1;
  const int n_items = n_img * (hwi / 2 / 8);
  return (int64_t)((n_items + 1) / 2) * (2 * cin * cin * 10);
}

extern "C" int sgmcmc_conv_down_bwd(const float* x, const float* w_main, const float* w_short,
                                    const float* dy_main, const float* dy_short, float* dx, float* dw_main,
                                    float* dw_short, float* scratch, int n_img, int cin, int hwi,
                                    int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w_main || !w_short || !dy_main || !dy_short || !dx || !scratch || n_img <= 0 ||
      (!deferred_slabs && (!dw_main || !dw_short)))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (cin == 16 && hwi == 32)
    return convdown::launch_bwd<16, 32>(x, w_main, w_short, dy_main, dy_short, dx, dw_main, dw_short, scratch,
                                        n_img, deferred_slabs, s);
  if (cin == 32 && hwi == 16)
    return convdown::launch_bwd<32, 16>(x, w_main, w_short, dy_main, dy_short, dx, dw_main, dw_short, scratch,
                                        n_img, deferred_slabs, s);
  return (int)hipErrorInvalidValue;
}

extern "C" int sgmcmc_conv_down_bwd_ex(const float* x, const float* w_main, const float* w_short,
                                       const float* dy_main, const float* dy_short, float* dx,
                                       const sgmcmc_conv_bwd_epilogue* epi, float* dw_main, float* dw_short,
                                       float* scratch, int n_img, int cin, int hwi, int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w_main || !w_short || !dy_main || !dy_short || !dx || !scratch || n_img <= 0 || !epi ||
      (!deferred_slabs && (!dw_main || !dw_short)))
    return (int)hipErrorInvalidValue;
  if (epi->e_dout || epi->e_out || !epi->s_partial) return (int)hipErrorInvalidValue;     // only the SUMS half exists here
  conv::BwdEpilogue E;
  if (const int bad = conv::epilogue_from_abi(epi, n_img, E)) return bad;
  hipStream_t s = (hipStream_t)stream;
  if (cin == 16 && hwi == 32)
    return convdown::launch_bwd<16, 32>(x, w_main, w_short, dy_main, dy_short, dx, dw_main, dw_short, scratch,
                                        n_img, deferred_slabs, s, E);
  if (cin == 32 && hwi == 16)
    return convdown::launch_bwd<32, 16>(x, w_main, w_short, dy_main, dy_short, dx, dw_main, dw_short, scratch,
                                        n_img, deferred_slabs, s, E);
  return (int)hipErrorInvalidValue;
}

// slices per channel of the SUMS partials sgmcmc_conv_down_bwd_ex leaves (the INPUT's channels: bands of 8 rows)
extern "C" int sgmcmc_conv_down_bwd_sum_slices(int n_img, int cin, int hwi) {
  if (!((cin == 16 && hwi == 32) || (cin == 32 && hwi == 16)) || n_img <= 0) return -1;
  return n_img * (hwi / 8);
}

extern "C" int sgmcmc_conv_down_stat_slices(int n_img, int cin, int hwi) {
  if (!((cin == 16 && hwi == 32) || (cin == 32 && hwi == 16)) || n_img <= 0) return -1;
  return n_img * (hwi / 2 / 8);
}

extern "C" int sgmcmc_conv_down_fwd(const float* x, const float* w_main, const float* w_short, float* y_main,
                                    float* y_short, double* stats_main, double* stats_short, int n_img,
                                    int cin, int hwi, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w_main || !w_short || !y_main || !y_short || n_img <= 0 || (stats_main == nullptr) != (stats_short == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (cin == 16 && hwi == 32)
    return convdown::launch_fwd<16, 32>(x, w_main, w_short, y_main, y_short, stats_main, stats_short, n_img, s);
  if (cin == 32 && hwi == 16)
    return convdown::launch_fwd<32, 16>(x, w_main, w_short, y_main, y_short, stats_main, stats_short, n_img, s);
  return (int)hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------------------
// The stem: 3 -> 16 channels, 3x3 / stride 1 / pad 1 on 32x32 images (google_resnet.py:96-100).  K = 27
// does not split into whole input-channel groups, so a k-step is 4 consecutive (ci, r, s) indices and
// every lane carries ITS tap offsets (7 of them; the 28th product is padded with a zero weight).  Only
// the weight gradient is needed backwards (the images take no gradient): N = the 27 taps in two tiles.
namespace convstem {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int CIN = 3, COUT = 16, HW = 32, ROWS = 8, WP = HW + 8, CS = (ROWS + 2) * WP + 16;  // 416
constexpr int K = 27, KSTEPS = 7, BANDS = HW / ROWS;

__device__ __forceinline__ void stage(float* __restrict__ in_s, const float* __restrict__ xi, int y0, int tid) {
  constexpr int V = HW / 4, ROWSH = ROWS + 2;
  for (int i = tid; i < CIN * ROWSH * V; i += 256) {
    const int v = i % V, ry = (i / V) % ROWSH, ci = i / (V * ROWSH);
    const int gy = y0 - 1 + ry;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gy >= 0 && gy < HW) val = *reinterpret_cast<const float4*>(xi + ((size_t)ci * HW + gy) * HW + 4 * v);
    *reinterpret_cast<float4*>(in_s + ci * CS + ry * WP + 4 + 4 * v) = val;
  }
  for (int i = tid; i < CIN * ROWSH * 2; i += 256) {
    const int side = i & 1, ry = (i >> 1) % ROWSH, ci = (i >> 1) / ROWSH;
    in_s[ci * CS + ry * WP + (side ? HW + 4 : 3)] = 0.f;
  }
}

__device__ __forceinline__ int tap_offset(int kidx) {  // LDS offset of tap kidx = (ci, r, s) relative to a pixel
  const int ci = kidx / 9, r = (kidx % 9) / 3, s = kidx % 3;
  return ci * CS + r * WP + s;
}

// (block `b` of the stem's own `n_blocks` = 4 per image)
template <bool STATS>
__device__ __forceinline__ void fwd_block(int b, int n_blocks, const float* __restrict__ x, const float* __restrict__ w,
                                          float* __restrict__ y, double* __restrict__ stats, int n_slices) {
  __shared__ float in_s[CIN * CS];
  __shared__ float red[128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = conv::xcd_remap<16>(b, n_blocks);
  const int band = bid % BANDS, img = bid / BANDS;
  const int y0 = band * ROWS;
  stage(in_s, x + (size_t)img * CIN * HW * HW, y0, tid);
  const int n = lane & 15, kq = lane >> 4;
  float breg[KSTEPS];
  int aoff[KSTEPS];
#pragma unroll
  for (int kk = 0; kk < KSTEPS; ++kk) {
    const int kidx = 4 * kk + kq;
    breg[kk] = kidx < K ? w[n * K + kidx] : 0.f;
    aoff[kk] = tap_offset(kidx < K ? kidx : 0);
  }
  __syncthreads();
  float s1 = 0.f;
  f32x4 vals[4];
  float* __restrict__ yo = y + ((size_t)img * COUT + n) * HW * HW;
#pragma unroll
  for (int t = 0; t < 4; ++t) {          // 16 tiles of 16 pixels per band, 4 per wave
    const int p = wave * 4 + t, yy = p >> 1, x0 = (p & 1) * 16;
    const int base = yy * WP + x0 + n + 3;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(in_s[base + aoff[kk]], breg[kk], acc, 0, 0, 0);
    sgmcmc_store4<4>(y, yo + (size_t)(y0 + yy) * HW + x0 + 4 * kq, acc[0], acc[1], acc[2], acc[3]);
    vals[t] = acc;
    if (STATS) s1 += (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
  if (STATS)
    conv::band_stats<4>(vals, s1, ROWS * HW, red, stats + (size_t)(img * BANDS + band) * 2, (size_t)n_slices * 2);
}

template <bool STATS>
__global__ __launch_bounds__(256) void fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                  float* __restrict__ y, double* __restrict__ stats,
                                                  int n_slices) {
  fwd_block<STATS>((int)blockIdx.x, (int)gridDim.x, x, w, y, stats, n_slices);
}

// The stem as the CARRIER of the trunk's weight fragments: it is the first launch of a gradient evaluation and reads no
// trunk weight, so behind its own n_own workgroups trail the blocks of up to SGMCMC_FRAG_JOBS fragment jobs
// (conv2::frag_block4: the buffers sgmcmc_conv3x3_prepare_weights would write, without its launch) -- the structure of
// conv3x3_bwd_kernel's riders.  The first consumer is a later launch: the kernel boundary is the synchronisation.
template <bool STATS>
__global__ __launch_bounds__(256) void fwd_frags_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        float* __restrict__ y, double* __restrict__ stats,
                                                        int n_slices, int n_own, int jobs_first, conv2::FragJobs J) {
  // (jobs_first: the fragment blocks lead the grid, padded to a multiple of 8 so that the stem's blocks keep their XCDs)
  const int n_lead = jobs_first ? (J.first_block[J.n] + 7) & ~7 : 0;
  const int b = (int)blockIdx.x - n_lead;
  if (b >= 0 && b < n_own) {
    fwd_block<STATS>(b, n_own, x, w, y, stats, n_slices);
    return;
  }
  const int r = jobs_first ? (int)blockIdx.x : b - n_own;
  if (r >= J.first_block[J.n]) return;      // padding
  int j = 0;
  while (j + 1 < J.n && r >= J.first_block[j + 1]) ++j;
  conv2::frag_block4(J.job[j], r - J.first_block[j]);
}

// dw[co][kidx] slabs: wave = pixel quarter of the band; per 4-pixel k-step one A fetch (dy) and two B
// fetches (taps 0..15, 16..26 of the lane's column)
__global__ __launch_bounds__(256) void wrw_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                  float* __restrict__ part, int n_items) {
  constexpr int NPIX = ROWS * HW, DS = NPIX + 4, ITEMS = 2;
  __shared__ float in_s[CIN * CS];
  __shared__ float dy_s[16 * DS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, kq = lane >> 4;
  const int off0 = tap_offset(n), off1 = tap_offset(16 + n < K ? 16 + n : 0);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const int bid = conv::xcd_remap<16>((int)blockIdx.x, (int)gridDim.x);      // (slab bid holds the items 2 bid, 2 bid + 1 as before)
  for (int it = 0; it < ITEMS; ++it) {
    const int item = bid * ITEMS + it;
    if (item >= n_items) break;
    const int band = item % BANDS, img = item / BANDS, y0 = band * ROWS;
    if (it) __syncthreads();
    const float* __restrict__ di = dy + (((size_t)img * COUT) * HW + y0) * HW;
    float4 rd[(16 * NPIX / 4 + 255) / 256];      // dy's loads are in flight while the (single-stripe) input is staged
    conv::stage_load<16 * NPIX / 4, float4>(rd, [&](int i) {
      const int v = i % (NPIX / 4), co = i / (NPIX / 4);
      return *reinterpret_cast<const float4*>(di + (size_t)co * HW * HW + 4 * v);
    });
    stage(in_s, x + (size_t)img * CIN * HW * HW, y0, tid);
    conv::stage_store<16 * NPIX / 4, float4>(rd, [&](int i, const float4& val) {
      const int v = i % (NPIX / 4), co = i / (NPIX / 4);
      *reinterpret_cast<float4*>(dy_s + co * DS + 4 * v) = val;
    });
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < NPIX / 16; ++kk) {
      const int g = wave * (NPIX / 16) + kk, row = g / (HW / 4), xg = g % (HW / 4);
      const float a = dy_s[n * DS + 4 * g + kq];
      const int pix = row * WP + 4 * xg + kq + 3;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, in_s[pix + off0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, in_s[pix + off1], acc1, 0, 0, 0);
    }
  }
  __syncthreads();
  float* __restrict__ red = dy_s;  // [wave][2][256]
  *reinterpret_cast<float4*>(red + (wave * 2) * 256 + 4 * lane) = make_float4(acc0[0], acc0[1], acc0[2], acc0[3]);
  *reinterpret_cast<float4*>(red + (wave * 2 + 1) * 256 + 4 * lane) = make_float4(acc1[0], acc1[1], acc1[2], acc1[3]);
  __syncthreads();
  for (int i = tid; i < 2 * 256; i += 256) {
    const int e = i % 256, tile = i / 256;
    const float v = (red[(0 * 2 + tile) * 256 + e] + red[(1 * 2 + tile) * 256 + e]) +
                    (red[(2 * 2 + tile) * 256 + e] + red[(3 * 2 + tile) * 256 + e]);
    const int ln = e >> 2, vv = e & 3, co = 4 * (ln >> 4) + vv, kidx = tile * 16 + (ln & 15);
    if (kidx < K) part[(size_t)bid * (COUT * K) + co * K + kidx] = v;
  }
}

}  // namespace convstem

extern "C" int sgmcmc_conv_stem_fwd(const float* x, const float* w, float* y, double* stats, int n_img,
                                    void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !y || n_img <= 0) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(n_img * convstem::BANDS)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (stats) SGMCMC_LAUNCH(convstem::fwd_kernel<true>, grid, block, 0, s, x, w, y, stats, n_img * convstem::BANDS);
  else SGMCMC_LAUNCH(convstem::fwd_kernel<false>, grid, block, 0, s, x, w, y, nullptr, 0);
  return (int)hipGetLastError();
}

// ... with the fragments of up to SGMCMC_FRAG_JOBS trunk convolutions prepared by trailing workgroups of the launch
extern "C" int sgmcmc_conv_stem_fwd_frags(const float* x, const float* w, float* y, double* stats, int n_img,
                                          const sgmcmc_frag_job* jobs, int n_jobs, int jobs_first, void* stream) {
  if (n_jobs == 0) return sgmcmc_conv_stem_fwd(x, w, y, stats, n_img, stream);
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !y || n_img <= 0 || !jobs || n_jobs < 0 || n_jobs > SGMCMC_FRAG_JOBS) return (int)hipErrorInvalidValue;
  conv2::FragJobs J;
  if (const int bad = conv2::frag_jobs_from_abi(jobs, n_jobs, conv2::frag_blocks4, J)) return bad;
  const int n_own = n_img * convstem::BANDS;
  const int first = jobs_first != 0, n_frag = first ? (J.first_block[n_jobs] + 7) & ~7 : J.first_block[n_jobs];
  const dim3 grid((unsigned)(n_own + n_frag)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (stats) SGMCMC_LAUNCH(convstem::fwd_frags_kernel<true>, grid, block, 0, s, x, w, y, stats, n_own, n_own, first, J);
  else SGMCMC_LAUNCH(convstem::fwd_frags_kernel<false>, grid, block, 0, s, x, w, y, nullptr, 0, n_own, first, J);
  return (int)hipGetLastError();
}

extern "C" int64_t sgmcmc_conv_stem_scratch_floats(int n_img) {
  return n_img <= 0 ? -1 : (int64_t)((n_img * convstem::BANDS + 1) / 2) * (convstem::COUT * convstem::K);
}

extern "C" int sgmcmc_conv_stem_wrw(const float* x, const float* dy, float* dw, float* scratch, int n_img,
                                    int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !dy || !scratch || n_img <= 0 || (!dw && !deferred_slabs)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int n_items = n_img * convstem::BANDS, P = (n_items + 1) / 2;
  SGMCMC_LAUNCH(convstem::wrw_kernel, dim3((unsigned)P), dim3(256), 0, s, x, dy, scratch, n_items);
  return conv::finish_slabs(deferred_slabs, P, s, {{scratch, convstem::COUT * convstem::K, dw, 1}});
}

// ------------------------------------------------------------------------------------------------
// The convolutional classifier's first layer (models/conv_nets.py:44-51): 1 -> 50 channels, 3x3 / stride 1 /
// pad 1 on 28x28 images, no bias here (it joins sgmcmc_bias_relu_pool_*).  K = 9 taps (3 k-steps, padded to
// 12 with zero weights); 50 output channels = 4 tiles of 16 (the last one 2 wide); pixel tiles are 16
// consecutive pixels of a 4-row band in row-major order (28 is not a multiple of 16: every lane carries
// its own row/column offset).  Only the weight gradient exists backwards.
namespace convfirst {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int COUT = 50, HW = 28, ROWS = 4, BANDS = HW / ROWS, WP = 36, CS = (ROWS + 2) * WP;
constexpr int K = 9, KSTEPS = 3, CT = 4, NPIX = ROWS * HW, NT = NPIX / 16;   // 112 pixels = 7 tiles per band

__device__ __forceinline__ void stage(float* __restrict__ in_s, const float* __restrict__ xi, int y0, int tid) {
  constexpr int V = HW / 4, ROWSH = ROWS + 2;
  for (int i = tid; i < ROWSH * V; i += 256) {
    const int v = i % V, ry = i / V, gy = y0 - 1 + ry;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gy >= 0 && gy < HW) val = *reinterpret_cast<const float4*>(xi + (size_t)gy * HW + 4 * v);
    *reinterpret_cast<float4*>(in_s + ry * WP + 4 + 4 * v) = val;
  }
  if (tid < ROWSH * 2) in_s[(tid >> 1) * WP + ((tid & 1) ? HW + 4 : 3)] = 0.f;
}

__device__ __forceinline__ int tap_offset(int kidx) { return (kidx / 3) * WP + kidx % 3; }

// ---- the first layer WITH its tail: conv -> + bias -> ReLU -> MaxPool2d(2) in one launch each way ---------------
// (conv_nets.py:46-57: Conv2d(1, 50, 3, padding=1), ReLU, MaxPool2d(2).)  The 50 x 28 x 28 map (20 MB per batch of
// 128) never reaches memory: the forward leaves the pooled 50 x 14 x 14 map and ONE BYTE per pooled element
// (conv::pool_window) and the backward rebuilds the band's dense dy in LDS from the pooled gradient and that byte
// (conv::unpool_window), then runs the same weight-gradient contraction (same operands, same order, same bits); the bias
// gradient's per-band partial sums leave with the slabs.
constexpr int YS = NPIX + 4, PW = HW / 2, PCELLS = (ROWS / 2) * PW;   // 28 pooled cells per channel and band

// The forward of one (image, band) workgroup.  POOL_EPI: the tiles go to LDS and leave through + bias -> ReLU ->
// MaxPool2d(2) as (pooled, code); else they are stored to y.
template <bool POOL_EPI>
__device__ __forceinline__ void fwd_body(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                         const float* __restrict__ bias, float* __restrict__ pooled,
                                         uint8_t* __restrict__ code) {
  const int bid = conv::xcd_remap((int)blockIdx.x, (int)gridDim.x);      // XCD-aware block order (round 6)
  __shared__ float in_s[CS];
  __shared__ __attribute__((aligned(16))) float y_s[POOL_EPI ? COUT * YS : 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int band = bid % BANDS, img = bid / BANDS, y0 = band * ROWS;
  stage(in_s, x + (size_t)img * HW * HW, y0, tid);
  const int n = lane & 15, kq = lane >> 4;
  int aoff[KSTEPS];
#pragma unroll
  for (int kk = 0; kk < KSTEPS; ++kk) aoff[kk] = tap_offset(4 * kk + kq < K ? 4 * kk + kq : 0);
  __syncthreads();
  // (pixel tile, channel tile) pairs round-robin over the waves: 7 x 4 = 28 pairs, 7 per wave
  for (int pair = wave; pair < NT * CT; pair += 4) {
    const int t = pair / CT, ct = pair % CT, co = ct * 16 + n;
    float breg[KSTEPS];
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) {
      const int kidx = 4 * kk + kq;
      breg[kk] = (kidx < K && co < COUT) ? w[co * K + kidx] : 0.f;
    }
    const int p = 16 * t + n, base = (p / HW) * WP + p % HW + 3;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(in_s[base + aoff[kk]], breg[kk], acc, 0, 0, 0);
    if (co < COUT) {   // D rows 4kq .. 4kq+3 = 4 consecutive pixels of the band (row-major: contiguous in memory)
      if constexpr (POOL_EPI)
        *reinterpret_cast<float4*>(y_s + co * YS + 16 * t + 4 * kq) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      else
        sgmcmc_store4<4>(y, y + ((size_t)img * COUT + co) * HW * HW + (size_t)y0 * HW + 16 * t + 4 * kq, acc[0], acc[1], acc[2], acc[3]);
    }
  }
  if constexpr (POOL_EPI) {
    __syncthreads();
    for (int i = tid; i < COUT * PCELLS; i += 256) {
      const int c = i / PCELLS, q = i % PCELLS, oi = q / PW, oj = q % PW;
      const float* __restrict__ src = y_s + c * YS + 2 * oi * HW + 2 * oj;
      const float2 r0 = *reinterpret_cast<const float2*>(src);
      const float2 r1 = *reinterpret_cast<const float2*>(src + HW);
      const size_t o = (((size_t)img * COUT + c) * PW + (y0 >> 1) + oi) * PW + oj;
      int k;
      pooled[o] = conv::pool_window(r0, r1, bias ? bias[c] : 0.f, &k);
      code[o] = (uint8_t)k;
    }
  }
}

__global__ __launch_bounds__(256) void fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                  float* __restrict__ y) {
  fwd_body<false>(x, w, y, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void fwd_pool_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ pooled,
                                                       uint8_t* __restrict__ code) {
  fwd_body<true>(x, w, nullptr, bias, pooled, code);
}

// dw[co][tap] slabs, one per (image, band): wave = channel tile; per 4-pixel k-step one A fetch (dy) and one B fetch
// (the lane's tap of x).  (One workgroup per image walking its 7 bands paid 7 serialised load latencies on half
// of the CUs: 16.4 us; a workgroup per band pays one.)  FROM_POOLED: dy is the gradient of the POOLED map and `code` its
// bytes -- the band's dense dy is rebuilt in LDS -- and dbias_part (may be NULL) takes the band's bias-gradient partials.
template <bool FROM_POOLED>
__device__ __forceinline__ void wrw_body(const float* __restrict__ x, const float* __restrict__ dy,
                                         const uint8_t* __restrict__ code, float* __restrict__ part,
                                         float* __restrict__ dbias_part) {
  const int bid = conv::xcd_remap((int)blockIdx.x, (int)gridDim.x);      // XCD-aware block order (round 6)
  constexpr int DS = NPIX + 4;
  __shared__ float in_s[CS];
  __shared__ __attribute__((aligned(16))) float dy_s[CT * 16 * DS];
  __shared__ float d_s[FROM_POOLED ? COUT * PCELLS : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int band = bid % BANDS, img = bid / BANDS, n = lane & 15, kq = lane >> 4;
  const int off = tap_offset(n < K ? n : 0), y0 = band * ROWS;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if constexpr (FROM_POOLED) {
    // the band's pooled gradients and bytes first (the only loads that the contraction waits for), x next to them
    constexpr int PER = (COUT * PCELLS + 255) / 256;
    float dreg[PER];
    uint8_t creg[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int i = tid + 256 * r;
      dreg[r] = 0.f;
      creg[r] = 0;
      if (i < COUT * PCELLS) {
        const int c = i / PCELLS, q = i % PCELLS;
        const size_t o = (((size_t)img * COUT + c) * PW + (y0 >> 1)) * PW + q;   // the band's two pooled rows: contiguous
        dreg[r] = dy[o];
        creg[r] = code[o];
      }
    }
    stage(in_s, x + (size_t)img * HW * HW, y0, tid);
    for (int i = tid; i < (CT * 16 - COUT) * DS; i += 256) dy_s[COUT * DS + i] = 0.f;     // the channel padding
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int i = tid + 256 * r;
      if (i < COUT * PCELLS) {
        const int c = i / PCELLS, q = i % PCELLS, oi = q / PW, oj = q % PW;
        d_s[i] = conv::unpool_window(dy_s + c * DS + 2 * oi * HW + 2 * oj, HW, dreg[r], creg[r]);
      }
    }
  } else {
    float4 rd[(CT * 16 * NPIX / 4 + 255) / 256];
    conv::stage_load<CT * 16 * NPIX / 4, float4>(rd, [&](int i) {
      const int v = i % (NPIX / 4), c = i / (NPIX / 4);
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < COUT)
        val = *reinterpret_cast<const float4*>(dy + ((size_t)img * COUT + c) * HW * HW + (size_t)y0 * HW + 4 * v);
      return val;
    });
    stage(in_s, x + (size_t)img * HW * HW, y0, tid);
    conv::stage_store<CT * 16 * NPIX / 4, float4>(rd, [&](int i, const float4& val) {
      const int v = i % (NPIX / 4), c = i / (NPIX / 4);
      *reinterpret_cast<float4*>(dy_s + c * DS + 4 * v) = val;
    });
  }
  __syncthreads();
#pragma unroll 4
  for (int g = 0; g < NPIX / 4; ++g) {
    const int p = 4 * g + kq;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dy_s[(wave * 16 + n) * DS + p],
                                               in_s[(p / HW) * WP + p % HW + 3 + off], acc, 0, 0, 0);
  }
  // D[row = co][col = tap]
  if (n < K) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int co = wave * 16 + 4 * kq + v;
      if (co < COUT) part[(size_t)bid * (COUT * K) + co * K + n] = acc[v];
    }
  }
  if constexpr (FROM_POOLED) {
    if (dbias_part && tid < COUT) {     // the band's share of the bias gradient: its 28 cells in order
      float sum = 0.f;
#pragma unroll 4
      for (int q = 0; q < PCELLS; ++q) sum += d_s[tid * PCELLS + q];
      dbias_part[(size_t)bid * COUT + tid] = sum;
    }
  }
}

__global__ __launch_bounds__(256) void wrw_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                  float* __restrict__ part) {
  wrw_body<false>(x, dy, nullptr, part, nullptr);
}

__global__ __launch_bounds__(256) void wrw_pool_kernel(const float* __restrict__ x, const float* __restrict__ dpooled,
                                                       const uint8_t* __restrict__ code, float* __restrict__ part,
                                                       float* __restrict__ dbias_part) {
  wrw_body<true>(x, dpooled, code, part, dbias_part);
}

}  // namespace convfirst

extern "C" int sgmcmc_conv_first_fwd(const float* x, const float* w, float* y, int n_img, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !y || n_img <= 0) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(convfirst::fwd_kernel, dim3((unsigned)(n_img * convfirst::BANDS)), dim3(256), 0,
                     (hipStream_t)stream, x, w, y);
  return (int)hipGetLastError();
}

extern "C" int64_t sgmcmc_conv_first_scratch_floats(int n_img) {
  return n_img <= 0 ? -1 : (int64_t)n_img * convfirst::BANDS * convfirst::COUT * convfirst::K;
}

extern "C" int sgmcmc_conv_first_wrw(const float* x, const float* dy, float* dw, float* scratch, int n_img,
                                     int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !dy || !scratch || n_img <= 0 || (!dw && !deferred_slabs)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int P = n_img * convfirst::BANDS;
  SGMCMC_LAUNCH(convfirst::wrw_kernel, dim3((unsigned)P), dim3(256), 0, s, x, dy, scratch);
  return conv::finish_slabs(deferred_slabs, P, s, {{scratch, convfirst::COUT * convfirst::K, dw, 1}});
}

/* conv_first + bias + ReLU + MaxPool2d(2) in one launch: pooled [n][50][14][14], code [n][50][14][14] bytes */
extern "C" int sgmcmc_conv_first_pool_fwd(const float* x, const float* w, const float* bias, float* pooled,
                                          uint8_t* code, int n_img, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !pooled || !code || n_img <= 0) return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(convfirst::fwd_pool_kernel, dim3((unsigned)(n_img * convfirst::BANDS)), dim3(256), 0,
                (hipStream_t)stream, x, w, bias, pooled, code);
  return (int)hipGetLastError();
}

extern "C" int64_t sgmcmc_conv_first_pool_scratch_floats(int n_img) {
  return n_img <= 0 ? -1 : (int64_t)n_img * convfirst::BANDS * convfirst::COUT * (convfirst::K + 1);
}

/* its backward: weight-gradient slabs [P][450] at scratch, bias-gradient slabs [P][50] behind them (P = n_img * 7
 * bands); dw / dbias reduced here, or -- deferred_slabs != NULL -- left to the caller's sgmcmc_wrw_reduce_many */
extern "C" int sgmcmc_conv_first_pool_bwd(const float* x, const float* dpooled, const uint8_t* code, float* dw,
                                          float* dbias, float* scratch, int n_img, int want_bias,
                                          int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !dpooled || !code || !scratch || n_img <= 0 || (!deferred_slabs && (!dw || (want_bias && !dbias))))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int P = n_img * convfirst::BANDS, E = convfirst::COUT * convfirst::K;
  float* bpart = want_bias ? scratch + (size_t)P * E : nullptr;
  SGMCMC_LAUNCH(convfirst::wrw_pool_kernel, dim3((unsigned)P), dim3(256), 0, s, x, dpooled, code, scratch, bpart);
  return conv::finish_slabs(deferred_slabs, P, s,
                            {{scratch, E, dw, 1}, {bpart, convfirst::COUT, want_bias ? dbias : nullptr, 1}});
}
