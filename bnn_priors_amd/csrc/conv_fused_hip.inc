// Backward of "convolution -> BatchNorm -> (+ shortcut) -> ReLU" with the BatchNorm's data gradient formed INSIDE
// the convolution's gradient launch (models/google_resnet.py:34-43, 77-90 inside inference.py:215-223).
//
// Layer by layer the backward of one such pair is   bn::bwd_sums -> bn::bwd_dx -> conv3x3_bwd   (+ an ATen add where
// the shortcut's gradient joins).  bwd_dx is pure element-wise work between two launches: here the convolution's
// gradient kernel reads what bwd_dx read (dout, the ReLU mask's tensor, the pre-BN activations) and forms
//
//     dy = k * (dz - mdb - xhat * mdg),   dz = dout * [out > 0],   xhat = (y - mean) * invstd,
//     k = gamma * invstd,  mdb = sum dz / M,  mdg = sum dz * xhat / M
//
// while it stages its operands into LDS -- for the data gradient's input band and for the weight gradient's dy
// tile alike -- so bwd_dx's launch, its read of three tensors and its write of dy disappear.  The per-channel
// sums come from bn::bwd_sums_kernel's per-slice partials (a separate launch: a grid-wide reduction needs a
// kernel boundary -- finishing it in-launch through tickets cost 7-12 us per hand-off on MI355X, measured, against
// ~1.5 us for the boundary); every workgroup combines the C x S <= 512 partial pairs itself, in slice order, while
// its operand loads are in flight.  The shortcut's gradient (dz of the block's LAST BatchNorm, = e_dout * [e_out > 0])
// is added in the data-gradient epilogue (EPI_ADD), which replaces the ATen add.
//
// Arithmetic: identical formulas to bn::bwd_dx_kernel; the weight-gradient slabs keep their fixed-order reduction.

namespace conv {

struct FusedBwd {
  const float* dout;       // gradient w.r.t. the BatchNorm's (post-ReLU) output
  const float* mask_out;   // that output (the ReLU mask: dz = dout * [mask_out > 0])
  const float* y;          // the BatchNorm's input = this convolution's forward output
  const float* mean;       // [C] saved batch mean
  const float* invstd;     // [C] saved 1 / sqrt(var + eps)
  const float* gamma;      // [C]
  const double* sums;      // [C][n_sums][2] per-slice (sum dz, sum dz * xhat) from bn::bwd_sums_kernel<true>
  int n_sums;
  double count;            // M = N * H * W
  float* dgamma;           // [C] out (written by workgroup 0)
  float* dbeta;            // [C] out
  const float* e_dout;     // EPI_ADD: dx += e_dout * [e_out > 0]
  const float* e_out;
};

// The BatchNorm backward's per-channel coefficients into LDS: bco[0][c] = k, bco[1][c] = mdb, bco[2][c] = mdg,
// bco[3][c] = mean, bco[4][c] = invstd, from the C x n_sums <= 512 partial pairs of bn::bwd_sums_kernel.
// Two phases so that no thread waits on a CHAIN of dependent global loads (a serial 32-term loop per channel
// cost ~6 us): bn_coefs_load -- every thread fetches at most two pairs (independent loads, issued while the
// operand loads are in flight); bn_coefs_finish -- the pairs go through `scratch` (8 KB of the not yet written
// operand area), four threads per channel add a quarter of the slices each in slice order, fixed shuffle tree.
// Workgroup 0 also writes dgamma / dbeta.  Ends with a barrier: bco complete, scratch free.
struct CoefLoad { double2 v0, v1; };

template <int C>
__device__ __forceinline__ CoefLoad bn_coefs_load(const FusedBwd& B) {
  const int t = threadIdx.x, total = C * B.n_sums;
  const double2* __restrict__ p = reinterpret_cast<const double2*>(B.sums);
  CoefLoad r;
  r.v0 = t < total ? p[t] : make_double2(0.0, 0.0);
  r.v1 = t + 256 < total ? p[t + 256] : make_double2(0.0, 0.0);
  return r;
}

template <int C>
__device__ __forceinline__ void bn_coefs_finish(const FusedBwd& B, const CoefLoad& r, float* __restrict__ bco,
                                                float* __restrict__ scratch_f) {
  double2* __restrict__ scr = reinterpret_cast<double2*>(scratch_f);
  const int t = threadIdx.x;
  scr[t] = r.v0;
  scr[t + 256] = r.v1;
  __syncthreads();
  if (t < 4 * C) {
    const int c = t >> 2, part = t & 3, per = (B.n_sums + 3) >> 2;
    double a = 0.0, b = 0.0;
    for (int s = part * per; s < min(B.n_sums, (part + 1) * per); ++s) { const double2 v = scr[c * B.n_sums + s]; a += v.x; b += v.y; }
    a += __shfl_xor(a, 1, 64); b += __shfl_xor(b, 1, 64);
    a += __shfl_xor(a, 2, 64); b += __shfl_xor(b, 2, 64);
    if (part == 0) {
      const float invstd = B.invstd[c];
      bco[c] = B.gamma[c] * invstd;
      bco[C + c] = (float)(a / B.count);
      bco[2 * C + c] = (float)(b / B.count);
      bco[3 * C + c] = B.mean[c];
      bco[4 * C + c] = invstd;
      if (blockIdx.x == 0) { B.dbeta[c] = (float)a; B.dgamma[c] = (float)b; }
    }
  }
  __syncthreads();
}

struct Dy4 { float4 dz, o, y; bool ok; };

__device__ __forceinline__ Dy4 load_dy(const FusedBwd& B, size_t off, bool ok) {
  Dy4 r;
  r.ok = ok;
  r.dz = r.o = r.y = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) {
    r.dz = *reinterpret_cast<const float4*>(B.dout + off);
    r.o = *reinterpret_cast<const float4*>(B.mask_out + off);
    r.y = *reinterpret_cast<const float4*>(B.y + off);
  }
  return r;
}
// (same expression as bn::bwd_dx_kernel)
template <int C>
__device__ __forceinline__ float4 finish_dy(const Dy4& r, const float* __restrict__ bco, int c) {
  if (!r.ok) return make_float4(0.f, 0.f, 0.f, 0.f);
  const float k = bco[c], mdb = bco[C + c], mdg = bco[2 * C + c], mean = bco[3 * C + c], invstd = bco[4 * C + c];
  const float d0 = r.o.x > 0.f ? r.dz.x : 0.f, d1 = r.o.y > 0.f ? r.dz.y : 0.f;
  const float d2 = r.o.z > 0.f ? r.dz.z : 0.f, d3 = r.o.w > 0.f ? r.dz.w : 0.f;
  float4 q;
  q.x = k * (d0 - mdb - ((r.y.x - mean) * invstd) * mdg);
  q.y = k * (d1 - mdb - ((r.y.y - mean) * invstd) * mdg);
  q.z = k * (d2 - mdb - ((r.y.z - mean) * invstd) * mdg);
  q.w = k * (d3 - mdb - ((r.y.w - mean) * invstd) * mdg);
  return q;
}

// ---- data gradient: conv3x3_body<TRANSPOSE_W> on dy, dy formed while staging
template <int C, int HW, int ROWS, bool EPI_ADD>
__device__ __forceinline__ void fused_dgrad_body(int b, const float* __restrict__ w, float* __restrict__ dx,
                                                 const FusedBwd& B, float* __restrict__ bco) {
  using G = Cfg<C, HW, ROWS>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* __restrict__ in_s = lds;
  float* __restrict__ w_s = lds + C * G::CS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = b % G::CT;
  b /= G::CT;
  const int band = b % G::BANDS, img = b / G::BANDS;
  const int y0 = band * ROWS;
  {
    constexpr int V = HW / 4, ROWSH = ROWS + 2;
    const size_t ibase = (size_t)img * C * HW * HW;
    float rw[(16 * G::K + 255) / 256];
    Dy4 rd[(C * ROWSH * V + 255) / 256];
    stage_load<16 * G::K, float>(rw, [&](int i) {
      const int n = i / G::K, kidx = i % G::K, co = kidx / 9, rs = kidx % 9;
      return w[((size_t)co * C + (ct * 16 + n)) * 9 + (8 - rs)];
    });
    stage_load<C * ROWSH * V, Dy4>(rd, [&](int i) {
      const int v = i % V, ry = (i / V) % ROWSH, ci = i / (V * ROWSH);
      const int gy = y0 - 1 + ry;
      return load_dy(B, ibase + ((size_t)ci * HW + gy) * HW + 4 * v, gy >= 0 && gy < HW);
    });
    const CoefLoad cl = bn_coefs_load<C>(B);      // its loads join the ones in flight
    stage_store<16 * G::K, float>(rw, [&](int i, float q) { w_s[(i / G::K) * G::KP + i % G::K] = q; });
    bn_coefs_finish<C>(B, cl, bco, in_s);         // (scratch: the input area, written only below)
    stage_store<C * ROWSH * V, Dy4>(rd, [&](int i, const Dy4& r) {
      const int v = i % V, ry = (i / V) % ROWSH, ci = i / (V * ROWSH);
      *reinterpret_cast<float4*>(in_s + ci * G::CS + ry * G::WP + 4 + 4 * v) = finish_dy<C>(r, bco, ci);
    });
    for (int i = tid; i < C * ROWSH * 2; i += 256) {
      const int side = i & 1, ry = (i >> 1) % ROWSH, ci = (i >> 1) / ROWSH;
      in_s[ci * G::CS + ry * G::WP + (side ? HW + 4 : 3)] = 0.f;
    }
  }
  __syncthreads();
  const int n = lane & 15, kq = lane >> 4;
  float breg[9][C / 4];
#pragma unroll
  for (int rs = 0; rs < 9; ++rs)
#pragma unroll
    for (int kk = 0; kk < C / 4; ++kk) breg[rs][kk] = w_s[n * G::KP + (4 * kk + kq) * 9 + rs];
  constexpr int NACC = G::PT_W == 1 ? 2 : G::PT_W;
  f32x4 acc[NACC];
  int abase[G::PT_W], orow[G::PT_W], ocol[G::PT_W];
#pragma unroll
  for (int t = 0; t < G::PT_W; ++t) {
    const int p = wave * G::PT_W + t;
    int yy, x0, m_y, m_x;
    if (HW >= 16) {
      constexpr int TPR = HW >= 16 ? HW / 16 : 1;
      yy = p / TPR; x0 = (p % TPR) * 16; m_y = 0; m_x = n;
    } else {
      yy = 2 * p; x0 = 0; m_y = n >> 3; m_x = n & 7;
    }
    abase[t] = kq * G::CS + (yy + m_y) * G::WP + x0 + m_x + 3;
    const int m0 = 4 * kq;
    if (HW >= 16) { orow[t] = yy; ocol[t] = x0 + m0; }
    else { orow[t] = yy + (m0 >> 3); ocol[t] = m0 & 7; }
  }
  // the epilogue's own operands: issued before the MFMA loop, consumed after it
  const size_t cbase = ((size_t)img * C + ct * 16 + n) * HW * HW;
  float4 ex[G::PT_W], ey[G::PT_W];
  if (EPI_ADD) {
#pragma unroll
    for (int t = 0; t < G::PT_W; ++t) {
      const size_t off = cbase + (size_t)(y0 + orow[t]) * HW + ocol[t];
      ex[t] = *reinterpret_cast<const float4*>(B.e_dout + off);
      ey[t] = *reinterpret_cast<const float4*>(B.e_out + off);
    }
  }
#pragma unroll
  for (int a = 0; a < NACC; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int rs = 0; rs < 9; ++rs) {
    const int r = rs / 3, s = rs % 3;
#pragma unroll
    for (int kk = 0; kk < C / 4; ++kk) {
#pragma unroll
      for (int t = 0; t < G::PT_W; ++t) {
        const float a = in_s[abase[t] + 4 * kk * G::CS + r * G::WP + s];
        const int ai = G::PT_W == 1 ? (kk & 1) : t;
        acc[ai] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, breg[rs][kk], acc[ai], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < G::PT_W; ++t) {
    f32x4 v = acc[t];
    if (G::PT_W == 1) v += acc[1];
    if (EPI_ADD) {
      v[0] += ey[t].x > 0.f ? ex[t].x : 0.f; v[1] += ey[t].y > 0.f ? ex[t].y : 0.f;
      v[2] += ey[t].z > 0.f ? ex[t].z : 0.f; v[3] += ey[t].w > 0.f ? ex[t].w : 0.f;
    }
    *reinterpret_cast<float4*>(dx + cbase + (size_t)(y0 + orow[t]) * HW + ocol[t]) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ---- weight gradient: conv3x3_wrw_body with its dy tile formed while staging
template <int C, int HW, int ROWS>
__device__ __forceinline__ void fused_wrw_body(int b, const float* __restrict__ x, float* __restrict__ part,
                                               const FusedBwd& B, int n_items, float* __restrict__ bco) {
  using G = WrwCfg<C, HW, ROWS, true>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* __restrict__ in_s = lds;
  float* __restrict__ dy_s = lds + C * G::CS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = b % G::CT, pw = b / G::CT;
  const int cit = wave % G::NCI, ps = wave / G::NCI;
  const int n = lane & 15, kq = lane >> 4;
  f32x4 acc[9];
#pragma unroll
  for (int rs = 0; rs < 9; ++rs) acc[rs] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < G::ITEMS; ++it) {
    const int item = pw * G::ITEMS + it;
    if (item >= n_items) break;
    const int band = item % G::BANDS, img = item / G::BANDS;
    const int y0 = band * ROWS;
    if (it) __syncthreads();
    {
      constexpr int V = HW / 4, ROWSH = ROWS + 2;
      const float* __restrict__ xi = x + (size_t)img * C * HW * HW;
      const size_t dbase = (((size_t)img * C + ct * 16) * HW + y0) * HW;
      float4 rx[(C * ROWSH * V + 255) / 256];
      Dy4 rd[(16 * G::NPIX / 4 + 255) / 256];
      stage_load<C * ROWSH * V, float4>(rx, [&](int i) {
        const int v = i % V, ry = (i / V) % ROWSH, ci = i / (V * ROWSH);
        const int gy = y0 - 1 + ry;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < HW) val = *reinterpret_cast<const float4*>(xi + ((size_t)ci * HW + gy) * HW + 4 * v);
        return val;
      });
      stage_load<16 * G::NPIX / 4, Dy4>(rd, [&](int i) {
        const int v = i % (G::NPIX / 4), co = i / (G::NPIX / 4);
        return load_dy(B, dbase + (size_t)co * HW * HW + 4 * v, true);
      });
      if (it == 0) {
        const CoefLoad cl = bn_coefs_load<C>(B);
        bn_coefs_finish<C>(B, cl, bco, in_s);     // (scratch: the input area, written only below)
      }
      stage_store<C * ROWSH * V, float4>(rx, [&](int i, const float4& val) {
        const int v = i % V, ry = (i / V) % ROWSH, ci = i / (V * ROWSH);
        *reinterpret_cast<float4*>(in_s + ci * G::CS + ry * G::WP + 4 + 4 * v) = val;
      });
      stage_store<16 * G::NPIX / 4, Dy4>(rd, [&](int i, const Dy4& r) {
        const int v = i % (G::NPIX / 4), co = i / (G::NPIX / 4);
        *reinterpret_cast<float4*>(dy_s + co * G::DS + 4 * v) = finish_dy<C>(r, bco, ct * 16 + co);
      });
      for (int i = tid; i < C * ROWSH * 2; i += 256) {
        const int side = i & 1, ry = (i >> 1) % ROWSH, ci = (i >> 1) / ROWSH;
        in_s[ci * G::CS + ry * G::WP + (side ? HW + 4 : 3)] = 0.f;
      }
    }
    __syncthreads();
    const float* __restrict__ bsrc = in_s + (cit * 16 + n) * G::CS + kq + 3;
    const float* __restrict__ asrc = dy_s + n * G::DS + kq;
#pragma unroll
    for (int kk = 0; kk < G::KSTEPS; ++kk) {
      const int g = ps * G::KSTEPS + kk;
      const int row = g / (HW / 4), xg = g % (HW / 4);
      const float a = asrc[4 * g];
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) {
        const float bv = bsrc[(row + rs / 3) * G::WP + 4 * xg + rs % 3];
        acc[rs] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[rs], 0, 0, 0);
      }
    }
  }
  __syncthreads();
  float* __restrict__ red = lds;
#pragma unroll
  for (int rs = 0; rs < 9; ++rs)
    *reinterpret_cast<float4*>(red + (wave * 9 + rs) * 256 + 4 * lane) =
        make_float4(acc[rs][0], acc[rs][1], acc[rs][2], acc[rs][3]);
  __syncthreads();
  float* __restrict__ out = part + (size_t)pw * (C * C * 9) + (size_t)ct * 16 * C;   // tap-major slab (conv_hip.inc)
  for (int i = tid; i < G::NCI * 9 * 256; i += 256) {
    const int e = i % 256, rs = (i / 256) % 9, ci_t = i / (256 * 9);
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < G::PS; ++q) v += red[((q * G::NCI + ci_t) * 9 + rs) * 256 + e];
    const int ln = e >> 2, vv = e & 3;
    const int co = 4 * (ln >> 4) + vv, ci = ci_t * 16 + (ln & 15);
    out[((size_t)rs * C + co) * C + ci] = v;
  }
}

// (two workgroups per CU, i.e. 2 waves per SIMD: at most 256 registers per lane)
template <int C, int HW, int ROWS, bool EPI_ADD>
__global__ __launch_bounds__(256, 2) void fused_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           float* __restrict__ dx, float* __restrict__ part,
                                                           FusedBwd B, int n_dgrad, int n_items) {
  __shared__ float bco[5 * C];
  const int b = (int)blockIdx.x;
  const int n_wrw = (int)gridDim.x - n_dgrad;     // the long weight-gradient blocks first (see conv3x3_bwd_kernel)
  if (b < n_wrw) fused_wrw_body<C, HW, ROWS>(b, x, part, B, n_items, bco);
  else fused_dgrad_body<C, HW, ROWS, EPI_ADD>(b - n_wrw, w, dx, B, bco);
}

template <int C, int HW, int ROWS>
int launch_fused_bwd(const float* x, const float* w, float* dx, float* part, const FusedBwd& B, int n_img,
                     int* n_slabs, hipStream_t s) {
  using G = WrwCfg<C, HW, ROWS, true>;
  using F = Cfg<C, HW, ROWS>;
  const int n_items = n_img * G::BANDS, P = (n_items + G::ITEMS - 1) / G::ITEMS;
  const int n_dgrad = n_img * F::BANDS * F::CT;
  const size_t lds = F::LDS_BYTES > G::LDS_BYTES ? F::LDS_BYTES : G::LDS_BYTES;
  auto k0 = fused_bwd_kernel<C, HW, ROWS, false>;
  auto k1 = fused_bwd_kernel<C, HW, ROWS, true>;
  static bool attr_done = false;
  if (!attr_done) {
    for (const void* k : {reinterpret_cast<const void*>(k0), reinterpret_cast<const void*>(k1)}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  const dim3 grid((unsigned)(n_dgrad + P * G::CT)), block(256);
  if (B.e_dout) SGMCMC_LAUNCH(k1, grid, block, lds, s, x, w, dx, part, B, n_dgrad, n_items);
  else SGMCMC_LAUNCH(k0, grid, block, lds, s, x, w, dx, part, B, n_dgrad, n_items);
  return finish_slabs(n_slabs, P, s, {});      // (always left to the caller: n_slabs is required)
}

}  // namespace conv

// ================================================================ C ABI
extern "C" int sgmcmc_conv3x3_bn_bwd(const float* x, const float* w, float* dx, float* scratch,
                                     const sgmcmc_conv_bn_bwd_args* A, int n_img, int channels, int hw, int* n_slabs,
                                     void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !dx || !scratch || !A || !n_slabs || n_img <= 0 || !A->dout || !A->mask_out || !A->y || !A->mean ||
      !A->invstd || !A->gamma || !A->sums || A->n_sums <= 0 || A->n_sums > 64 || !A->dgamma || !A->dbeta ||
      (A->e_dout == nullptr) != (A->e_out == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  conv::FusedBwd B;
  B.dout = A->dout; B.mask_out = A->mask_out; B.y = A->y; B.mean = A->mean; B.invstd = A->invstd; B.gamma = A->gamma;
  B.sums = A->sums; B.n_sums = A->n_sums; B.count = (double)n_img * hw * hw; B.dgamma = A->dgamma; B.dbeta = A->dbeta;
  B.e_dout = A->e_dout; B.e_out = A->e_out;
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_fused_bwd<C, HW, ROWS>(x, w, dx, scratch, B, n_img, n_slabs, s));
}
