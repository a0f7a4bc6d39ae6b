// 3x3 / stride 1 / pad 1 convolutions of the ResNet trunk (C -> C channels, C in {16, 32, 64},
// square images of 32 / 16 / 8 pixels, NCHW fp32) as implicit GEMMs on the fp32 matrix pipe
// (v_mfma_f32_16x16x4_f32: exact f32, an fmaf chain per output).  Reference: the gradient of
// R1 (inference.py:215-223) through models/google_resnet.py:34-43's convolutions.
//
//   forward        y[n,co,p]   = sum_{ci,r,s} x[n,ci,p+(r-1,s-1)] * w[co,ci,r,s]
//   data gradient  dx[n,ci,p]  = sum_{co,r,s} dy[n,co,p-(r-1,s-1)] * w[co,ci,r,s]
//                  = the forward kernel on dy with w'[ci,co,r,s] = w[co,ci,2-r,2-s]   (TRANSPOSE_W)
//   weight gradient dw[co,ci,r,s] = sum_{n,p} dy[n,co,p] * x[n,ci,p+(r-1,s-1)]       (wrw kernels)
//
// Forward tiling: one workgroup = (image, band of ROWS rows, 16 output channels); the input band
// with its halo ([C][ROWS+2][W+8], interior 16-byte aligned) and the 16 x 9C weight slab are staged
// in LDS; each of the 4 waves keeps ITS B operands (the weight slab in MFMA layout, 9C/4 registers)
// resident and walks its pixel tiles (16 consecutive pixels) with ONE ds_read_b32 per MFMA for the
// A operand.  GEMM view per tile: M = 16 pixels, N = 16 channels, K = 9C.
// 512 workgroups per launch at batch 128 for all three stages (2 per CU), 144 MFMAs per wave.

namespace conv {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// Lab builds only (-DSGMCMC_STAMPS, tools/lab/bwd_timeline.py): wall-clock stamps (10 ns ticks) of a workgroup's phases
// in the merged backward launch, and where it ran -- never part of the product library.
#ifdef SGMCMC_STAMPS
__device__ unsigned long long g_stamps[4096 * 8];
__device__ __forceinline__ void stamp(int k) {
  if (threadIdx.x == 0) {
    if (k == 7) {
      unsigned hw;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      g_stamps[blockIdx.x * 8 + 7] = ((unsigned long long)([] { int v; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v)); return (unsigned)(v & 7); })() << 32) | hw;
    } else {
      g_stamps[blockIdx.x * 8 + k] = wall_clock64();
    }
  }
}
#define SGMCMC_STAMP(k) stamp(k)
#else
#define SGMCMC_STAMP(k)
#endif

// XCD-aware block order.  Workgroup ids are dealt round-robin to the 8 XCDs (id mod 8), each with its own L2; the
// work items of these kernels are ordered (image, band, channel tile), so consecutive ids -- the channel tiles of
// one band, the bands of one image -- share their input.  Dealing them to 8 different L2s made every XCD fetch the
// same band from the fabric (2.6-3.9x the algorithmic HBM reads at 64 channels, profiles/r02_conv_kernels_pmc_hbm.txt).
// remap: XCD r works through the CONTIGUOUS range [r n/8, (r+1) n/8) of items, so an image's tiles, bands and (in the
// merged backward launch) both of its gradients meet in one L2.  Pure relabelling: every item is computed exactly as
// before, by another workgroup -- results are bit-identical.  (n not a multiple of 8: identity.)
template <int C = 64>
__device__ __forceinline__ int xcd_remap(int b, int n) {
  return (n & 7) ? b : (b & 7) * (n >> 3) + (b >> 3);
}

// Two-phase operand staging: ALL of a thread's global loads are issued before its first LDS store, so a
// workgroup pays one memory latency per operand SET instead of one per 256-element stripe (a plain
// `for (i = tid; i < n; i += 256) lds[f(i)] = src[g(i)]` compiles to load -> s_waitcnt vmcnt(0) -> ds_write per
// iteration: 14 serialised round trips in the forward kernel, measured 5.6-7.5 us of a 12 us launch).
// stage2 keeps two operands' loads in flight together (e.g. the weight slab and the input band).
template <int TOTAL, typename V, typename Ld>
__device__ __forceinline__ void stage_load(V (&r)[(TOTAL + 255) / 256], Ld ld) {
#pragma unroll
  for (int it = 0; it < (TOTAL + 255) / 256; ++it) {
    const int i = (int)threadIdx.x + it * 256;
    if ((TOTAL % 256 == 0) || i < TOTAL) r[it] = ld(i);
  }
}
template <int TOTAL, typename V, typename St>
__device__ __forceinline__ void stage_store(const V (&r)[(TOTAL + 255) / 256], St st) {
#pragma unroll
  for (int it = 0; it < (TOTAL + 255) / 256; ++it) {
    const int i = (int)threadIdx.x + it * 256;
    if ((TOTAL % 256 == 0) || i < TOTAL) st(i, r[it]);
  }
}
template <int TOTAL, typename V, typename Ld, typename St>
__device__ __forceinline__ void stage(Ld ld, St st) {
  V r[(TOTAL + 255) / 256];
  stage_load<TOTAL, V>(r, ld);
  stage_store<TOTAL, V>(r, st);
}
template <int T1, typename V1, int T2, typename V2, typename Ld1, typename St1, typename Ld2, typename St2>
__device__ __forceinline__ void stage2(Ld1 ld1, St1 st1, Ld2 ld2, St2 st2) {
  V1 r1[(T1 + 255) / 256];
  V2 r2[(T2 + 255) / 256];
  stage_load<T1, V1>(r1, ld1);
  stage_load<T2, V2>(r2, ld2);
  stage_store<T1, V1>(r1, st1);
  stage_store<T2, V2>(r2, st2);
}

// Per-channel batch statistics of a workgroup's output band, from the accumulators: channel n lives in
// lanes n, n+16, n+32, n+48 of every wave (fixed xor tree), the 4 waves are added in order.  Two passes
// over the registers: the band's sum, then the squared deviations from the band's OWN mean -- the
// BatchNorm combines (sum, M2) pairs with Chan's formula, so nothing ever cancels against mean^2.
// dst[c * stride + {0, 1}] = (sum, M2) of channel c (16 channels); `lds`: 128 floats, free to use.
template <int NT>
__device__ __forceinline__ void band_stats(const f32x4 (&vals)[NT], float s1, int band_elems,
                                           float* __restrict__ lds, double* __restrict__ dst, size_t stride) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15;
  s1 += __shfl_xor(s1, 16, 64);
  s1 += __shfl_xor(s1, 32, 64);
  __syncthreads();                      // every wave is done reading the operand tiles
  if (lane < 16) lds[wave * 16 + lane] = s1;
  __syncthreads();
  const float tot = (lds[n] + lds[16 + n]) + (lds[32 + n] + lds[48 + n]);
  const float mean = tot / (float)band_elems;
  float s2 = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float d0 = vals[t][0] - mean, d1 = vals[t][1] - mean, d2 = vals[t][2] - mean, d3 = vals[t][3] - mean;
    s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  s2 += __shfl_xor(s2, 16, 64);
  s2 += __shfl_xor(s2, 32, 64);
  if (lane < 16) lds[64 + wave * 16 + lane] = s2;
  __syncthreads();
  if (tid < 16) {
    // M2 around the exact band mean mu = S / n from deviations around the rounded one:
    // sum (x - mu)^2 = sum (x - m)^2 - n (mu - m)^2
    const double S = ((double)lds[tid] + (double)lds[16 + tid]) + ((double)lds[32 + tid] + (double)lds[48 + tid]);
    const double Q = ((double)lds[64 + tid] + (double)lds[80 + tid]) + ((double)lds[96 + tid] + (double)lds[112 + tid]);
    const double m = (double)(((lds[tid] + lds[16 + tid]) + (lds[32 + tid] + lds[48 + tid])) / (float)band_elems);
    const double dm = S / band_elems - m;
    dst[(size_t)tid * stride] = S;
    dst[(size_t)tid * stride + 1] = Q - band_elems * dm * dm;
  }
}

// ---- a grid-wide sum without partial slabs: integer atomics into per-XCD slots -------------------------------------
// A workgroup adds its fp64 partial as two int64 limbs (multiples of 2^-8, and the remainder in units of 2^-60) to the
// slot of the XCD it runs on; the consumer adds the 8 slots AS INTEGERS -- commutative, so the total has the same bits
// whichever workgroup ran where and in whatever order -- and converts once.  Measured (tools/conv_lab/atom.hip): 64
// such atomics per workgroup cost nothing against 32 partial stores when each channel's limbs own a 128-byte line and
// the slot is per XCD; a device-wide slot set costs 3-19 us.  The caller hands out ZEROED slots (conv.fx_take).
// Layout: fx[slot][limb][channel][LINE] int64, limb = {0, 1}: quantity 0 (hi, lo), {2, 3}: quantity 1, {4}: non-finite
// count -- every (limb, channel) in its own 128-byte line (with a channel's four limbs in ONE line the 64 workgroups of
// an XCD queue up on it: +2.5 us per launch at 16 channels, measured in the step).
namespace fx {
constexpr int SLOTS = 8, LIMBS = 5, LINE = 16;
__device__ __forceinline__ int xcc() {
  int v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & (SLOTS - 1);
}
__device__ __forceinline__ size_t at(int slot, int limb, int C, int c) { return (((size_t)slot * LIMBS + limb) * C + c) * LINE; }
// channel c of THIS XCD's slot
__device__ __forceinline__ void add(long long* __restrict__ base, int C, int c, int q, double v) {
  const int slot = xcc();
  if (!(fabs(v) < 0x1p54)) {            // NaN, infinity, or beyond the coarse limb's range: the total becomes NaN
    __hip_atomic_fetch_add(base + at(slot, 4, C, c), 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const double coarse = rint(v * 256.0);
  const long long hi = (long long)coarse, lo = (long long)rint((v - coarse * 0x1p-8) * 0x1p60);
  __hip_atomic_fetch_add(base + at(slot, 2 * q, C, c), hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(base + at(slot, 2 * q + 1, C, c), lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// both quantities of channel c over all slots: `load` early (every load issued at once), `finish` where they are needed
struct Totals { long long v[SLOTS][LIMBS]; };
__device__ __forceinline__ Totals load(const long long* __restrict__ base, int C, int c) {
  Totals t;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s)
#pragma unroll
    for (int k = 0; k < LIMBS; ++k) t.v[s][k] = base[at(s, k, C, c)];
  return t;
}
__device__ __forceinline__ void finish(const Totals& t, double& q0, double& q1) {
  long long a[LIMBS] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < SLOTS; ++s)
#pragma unroll
    for (int k = 0; k < LIMBS; ++k) a[k] += t.v[s][k];
  q0 = (double)a[0] * 0x1p-8 + (double)a[1] * 0x1p-60;
  q1 = (double)a[2] * 0x1p-8 + (double)a[3] * 0x1p-60;
  if (a[4] != 0) q0 = q1 = __builtin_nan("");
}
}  // namespace fx

// band_stats with the band's (sum y, sum y^2) added to the channels' fx lines instead of stored per slice:
// sum y^2 = M2 around the band's exact mean + S^2 / n, all in double (the consumer forms var = E[y^2] - mean^2 from
// totals that are exact to 2^-60 per band, in double: what cancels is far below fp32's precision).
template <int NT>
__device__ __forceinline__ void band_stats_fx(const f32x4 (&vals)[NT], float s1, int band_elems,
                                              float* __restrict__ lds, long long* __restrict__ fxp, int C, int c0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15;
  s1 += __shfl_xor(s1, 16, 64);
  s1 += __shfl_xor(s1, 32, 64);
  __syncthreads();
  if (lane < 16) lds[wave * 16 + lane] = s1;
  __syncthreads();
  const float tot = (lds[n] + lds[16 + n]) + (lds[32 + n] + lds[48 + n]);
  const float mean = tot / (float)band_elems;
  float s2 = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float d0 = vals[t][0] - mean, d1 = vals[t][1] - mean, d2 = vals[t][2] - mean, d3 = vals[t][3] - mean;
    s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  s2 += __shfl_xor(s2, 16, 64);
  s2 += __shfl_xor(s2, 32, 64);
  if (lane < 16) lds[64 + wave * 16 + lane] = s2;
  __syncthreads();
  if (tid < 16) {
    const double S = ((double)lds[tid] + (double)lds[16 + tid]) + ((double)lds[32 + tid] + (double)lds[48 + tid]);
    const double Q = ((double)lds[64 + tid] + (double)lds[80 + tid]) + ((double)lds[96 + tid] + (double)lds[112 + tid]);
    const double m = (double)(((lds[tid] + lds[16 + tid]) + (lds[32 + tid] + lds[48 + tid])) / (float)band_elems);
    const double dm = S / band_elems - m;
    const double M2 = Q - band_elems * dm * dm;
    fx::add(fxp, C, c0 + tid, 0, S);
    fx::add(fxp, C, c0 + tid, 1, M2 + S * S / band_elems);
  }
}

// MEASURED, NOT THE DEFAULT (resblock.FOLD_BN): correct and bit-reproducible, but no faster -- in the googleresnet step
// the producer's atomics cost +1.3 / +0.5 / +0.1 us per launch at 16 / 32 / 64 channels (a line per limb; +2.5 / +1.2 /
// +0.4 with a channel's limbs in one line), the consumer +4.1 / +4.2 / +6.4 us (of which the side output h 1.1 / 0.6 /
// 0 us; the rest is the prologue -- 40 lines per channel to gather, 80 more registers -- on the critical path of the
// staging), against 5.8 / 4.9 / 4.6 us for the apply launch they replace: 1,183 steps/s either way.
// BNIN: the convolution's INPUT is relu(BatchNorm(x)) of the tensor it is given -- a residual block's first BatchNorm +
// ReLU applied while the operands are staged (google_resnet.py:34-43), its batch statistics taken from the producing
// convolution's fx slots.  The workgroup (image 0, band 0, tile 0) publishes the saved / running statistics exactly as
// bn::apply_kernel does; every workgroup writes its band's rows of its own 16 channels of h = relu(bn(x)) (the
// backward needs h), so the BatchNorm's apply launch, and its read of x, disappear.
struct BnIn {
  const long long* fx;
  const float* gamma;
  const float* beta;
  float* save_mean;
  float* save_invstd;
  float* running_mean;   // NULL with stat_log
  float* running_var;
  double* stat_log;      // logging mode, else NULL
  double momentum, eps, count;
  float* h;
};

// Per-channel partial sums of a workgroup's output band for the BatchNorm BACKWARD that consumes this output as its
// incoming gradient (SUMS epilogue of the data gradient): lane partials s1 = sum dz, s2 = sum dz * xhat of channel n
// -> lanes n, n+16, n+32, n+48 (fixed xor tree) -> the 4 waves in order, in double.  dst[c * stride + {0, 1}].
__device__ __forceinline__ void band_sums(float s1, float s2, float* __restrict__ lds, double* __restrict__ dst,
                                          size_t stride) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s1 += __shfl_xor(s1, 16, 64); s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 16, 64); s2 += __shfl_xor(s2, 32, 64);
  __syncthreads();                      // every wave is done reading the operand tiles
  if (lane < 16) { lds[wave * 16 + lane] = s1; lds[64 + wave * 16 + lane] = s2; }
  __syncthreads();
  if (tid < 16) {
    dst[(size_t)tid * stride] = ((double)lds[tid] + (double)lds[16 + tid]) + ((double)lds[32 + tid] + (double)lds[48 + tid]);
    dst[(size_t)tid * stride + 1] =
        ((double)lds[64 + tid] + (double)lds[80 + tid]) + ((double)lds[96 + tid] + (double)lds[112 + tid]);
  }
}

// ---- + bias -> ReLU -> MaxPool2d(2): ONE 2 x 2 window, for every kernel that pools (pool_hip.inc, convfirst, conv50) ----
// pool_window: the window's rows r0, r1 and the channel's bias -> relu(max + bias) and the window's byte: bits 0-1 the
// position of the FIRST maximum in scan order (0,0), (0,1), (1,0), (1,1) -- strict comparisons, NaNs win and propagate,
// as ATen's max_pool2d / relu -- bit 2 whether max + bias passed the ReLU.
__device__ __forceinline__ float pool_window(const float2 r0, const float2 r1, float bias, int* code) {
  float m = r0.x;
  int k = 0;
  if (r0.y > m || r0.y != r0.y) { m = r0.y; k = 1; }
  if (r1.x > m || r1.x != r1.x) { m = r1.x; k = 2; }
  if (r1.y > m || r1.y != r1.y) { m = r1.y; k = 3; }
  const float tv = m + bias;
  *code = k | (tv > 0.f ? 4 : 0);
  return tv > 0.f ? tv : (tv != tv ? tv : 0.f);
}
// ... and its inverse: the window of the gradient, written whole (rows `pitch` apart) -- the pooled cell's gradient at
// the position the byte names if that cell passed the ReLU, zeros elsewhere; -> the gradient that was routed
__device__ __forceinline__ float unpool_window(float* __restrict__ dst, int pitch, float dpooled, int code) {
  const float d = (code & 4) ? dpooled : 0.f;
  const int k = code & 3;
  *reinterpret_cast<float2*>(dst) = make_float2(k == 0 ? d : 0.f, k == 1 ? d : 0.f);
  *reinterpret_cast<float2*>(dst + pitch) = make_float2(k == 2 ? d : 0.f, k == 3 ? d : 0.f);
  return d;
}

// what the data gradient's epilogue may do besides storing dx (all pointers device; null = not requested)
struct BwdEpilogue {
  const float* e_dout;    // ADD: dx += e_dout * [e_out > 0]  (identity shortcut's gradient); e_out NULL: e_dout arrives
  const float* e_out;     //      masked already (its producer ran with mask_dx) and is added as it is
  const float* s_y;       // SUMS: the BatchNorm whose OUTPUT gradient dx is: its input y, its output (ReLU mask),
  const float* s_out;     //       saved mean / invstd; partial[(c * n_slices + slice) * 2 + {0,1}] <- sum dz, sum dz*xhat
  const float* s_mean;    //       over this workgroup's band, dz = dx * [s_out > 0]
  const float* s_invstd;
  double* s_partial;
  int n_slices;
  int group_imgs;         // > 0: groups of this many images, s_mean / s_invstd are [group][C] (bn_hip.inc, GROUPS)
  float inv_group_imgs;   // 1 / group_imgs, 0 for one batch (set by set_groups)
  int wrw_mult;           // > 1: a weight-gradient workgroup walks ITEMS x wrw_mult items (launches that carry several
                          //      minibatches: as many slabs as one minibatch leaves, each the sum over more images)
  int mask_dx;            // SUMS: dx is STORED as dz = dx * [s_out > 0] -- what both of its consumers (the BatchNorm's dx
                          //      launch, the shortcut add of the block before) would form from it: neither reads s_out again
};
// where the saved statistics of image `img`'s group start.  No integer division: its expansion in the sums epilogue
// cost the convolution-gradient kernels 30-90 VGPRs and a wave of occupancy (+1.2 us per launch in the leapfrog step);
// (img + 0.5) * (1 / group_imgs) is at least 0.5 / group_imgs away from an integer, far beyond float rounding for the
// <= 2^16 images of a launch.
__device__ __forceinline__ int group_offset(const BwdEpilogue* E, int img, int C) {
  // (uniform over the workgroup: back into a scalar register, the float detour must not hold a vector register)
  return __builtin_amdgcn_readfirstlane((int)(((float)img + 0.5f) * E->inv_group_imgs)) * C;
}

inline void set_groups(BwdEpilogue& E, int group_imgs) {
  E.group_imgs = group_imgs;
  E.inv_group_imgs = group_imgs > 0 ? 1.0f / (float)group_imgs : 0.0f;
}

// Evaluation mode (round 4): y = relu?(BN_eval(conv(x)) [+ residual]) in the convolution's epilogue -- with running
// statistics a BatchNorm is a per-channel affine map of the accumulator tile that is still in registers, so the
// BatchNorm launch, its read of the convolution's output and that output itself disappear from every test-set forward
// (inference.py:199-213, exp_utils.py:250-340).  bn::eval_kernel's arithmetic, operation for operation: the same bits.
struct EvalBn {
  const float* gamma;
  const float* beta;
  const float* mean;      // running statistics
  const float* var;
  const float* residual;  // may be NULL
  float eps;
  int relu;
};

// Row pitch of the weight slab in LDS.  Lane (n, kq) fills its B registers from w_s[n * pitch + (4 kk + kq) * 9 + rs];
// ds_read_b32 serves lanes 0-31 (kq = 0, 1) in one pass over 32 banks: bank = n * pitch + 9 kq.  With the round-1 pitch
// 9C + 1 (= 17 mod 32) nine of the sixteen n collided across the two kq; pitch = 2 mod 32 puts kq = 0 on the even and
// kq = 1 on the odd banks: conflict free (round 5: forward -0.1 / -0.2 / -0.35 us at 16 / 32 / 64 channels, the 64-channel
// gradients -0.2 ... -0.9 us; same bits).
template <int C, int HW, int ROWS>
struct Cfg {
  static constexpr int WP = HW + 8;  // row pitch: 4 pad | W interior | 4 pad (halo at 3 and W+4)
  static constexpr int CS_RAW = (ROWS + 2) * WP;
  // channel stride: the 4 k-lanes of an A fetch read 4 channels; keep their 16-dword runs in
  // different bank quarters (stride % 64 in {16, 48}) where the geometry allows it.
  // 8-pixel rows: a k-lane reads two runs of 8 (rows WP = 16 dwords apart); ds_read_b32 serves lanes 0-31 (k-lanes
  // 0, 1) and 32-63 (k-lanes 2, 3) in separate passes over 32 banks: stride = 8 mod 32 puts the second k-lane's runs
  // into the gaps of the first (banks b..b+7, b+16..b+23 | b+8..b+15, b+24..b+31) -- conflict free (round 3)
  static constexpr int CS = HW < 16 ? CS_RAW + ((8 - CS_RAW % 32) % 32 + 32) % 32
                            : (CS_RAW % 64 == 16 || CS_RAW % 64 == 48) ? CS_RAW
                            : CS_RAW + ((16 - CS_RAW % 64) % 64 + 64) % 64;
  static constexpr int K = 9 * C, KP = K + ((2 - K % 32) % 32 + 32) % 32;      // = 2 mod 32
  static constexpr int PT = ROWS * HW / 16;  // pixel tiles per workgroup
  static constexpr int PT_W = PT / 4;        // per wave
  static constexpr int BANDS = HW / ROWS, CT = C / 16;
  static constexpr size_t LDS_BYTES = (size_t)(C * CS + 16 * KP) * sizeof(float);
  static_assert(PT % 4 == 0 && PT_W >= 1, "4 waves share the pixel tiles");
};

// STATS: the epilogue also leaves this workgroup's per-channel (sum y, sum (y - band mean)^2) over its band
// in stats[(channel * n_slices + slice) * 2 + {0,1}], slice = img * BANDS + band -- the batch statistics the
// BatchNorm that follows needs (bn_hip.inc combines the slices), for free: y is still in registers.
// EPI (data gradient of a residual block's first convolution): y += e_dout * [e_out > 0] in the epilogue -- what the
// shortcut carries back to the block's input (replaces an ATen add and the dz tensor it would read).
// SUMS: the epilogue also leaves the partial sums the NEXT BatchNorm backward needs (band_sums above), from the
// registers -- the separate sums launch of that BatchNorm (5 us, 21 per step) disappears.
// FRAG != 0: `w` is not the raw [co][ci][3][3] tensor but its PREPARED FRAGMENTS (conv2::weight_frag_kernel's layout:
// forward order, or transposed + flipped with TRANSPOSE_W -- the permutation was done once per gradient evaluation, not
// by each of the launch's 512 workgroups).  Tile ct is 9C/16 float4 per lane, float4 f of lane l at
// w[((ct * 9C/16 + f) * 64 + l) * 4]; with KS = 2 at 64 channels, else 1, KK = C / 4 / KS, f = h * (9 KK / 4) + q4:
// component j is breg[rs][h * KK + k2], (rs, k2) = ((4 q4 + j) / KK, (4 q4 + j) % KK) -- the SAME register values as
// the raw route's fill, so the same bits.  FRAG_LDS: the tile is copied to LDS linearly (16-byte loads and stores) and
// every lane fills its registers with 9C/16 ds_read_b128; FRAG_REG: 9C/16 16-byte global loads straight into the
// registers, the slab's LDS stays unused.
constexpr int FRAG_LDS = 1, FRAG_REG = 2;
template <int C, int HW, int ROWS, bool TRANSPOSE_W, bool STATS, bool EPI = false, bool SUMS = false, bool BNIN = false,
          bool AFF = false, int FRAG = 0>
__device__ __forceinline__ void conv3x3_body(int b, const float* __restrict__ x, const float* __restrict__ w,
                                             float* __restrict__ y, double* __restrict__ stats,
                                             int n_slices, const BwdEpilogue* E = nullptr,
                                             long long* __restrict__ fx_out = nullptr, const BnIn* B = nullptr,
                                             const EvalBn* V = nullptr) {
  using G = Cfg<C, HW, ROWS>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* __restrict__ in_s = lds;
  float* __restrict__ w_s = lds + C * G::CS;
  float* __restrict__ bco = lds + C * G::CS + 16 * G::KP;      // BNIN: [3][C] mean, scale, shift (beyond LDS_BYTES)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = b % G::CT;
  b /= G::CT;
  const int band = b % G::BANDS, img = b / G::BANDS;
  const int y0 = band * ROWS;
  SGMCMC_STAMP(0);
  SGMCMC_STAMP(7);
  static_assert(!FRAG || !BNIN, "the fragment route does not fold a BatchNorm into its staging");
  constexpr int NF = 9 * C / 16;                      // FRAG: float4 per lane of a tile's fragments
  float4 fr[FRAG == FRAG_REG ? NF : 1];

  // ---- operands: the 16 x K weight slab (K ordered (ci, r, s) as in memory) and the input band with its halo,
  // every global load of both in flight before the first LDS store
  {
    constexpr int V = HW / 4, ROWSH = ROWS + 2;
    const float* __restrict__ xi = x + (size_t)img * C * HW * HW;
    auto slab_at = [](int e) { return (e / G::K) * G::KP + e % G::K; };      // element e = n * 9C + kidx of the row-major slab
    auto ld_in = [&](int i) {
      const int v = i % V, ry = (i / V) % ROWSH, ci = i / (V * ROWSH);
      const int gy = y0 - 1 + ry;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gy >= 0 && gy < HW) val = *reinterpret_cast<const float4*>(xi + ((size_t)ci * HW + gy) * HW + 4 * v);
      return val;
    };
    auto st_in = [&](int i, float4 val) {
      const int v = i % V, ry = (i / V) % ROWSH, ci = i / (V * ROWSH);
      if (BNIN) {
        const int gy = y0 - 1 + ry;
        if (gy >= 0 && gy < HW) {            // (rows outside the image stay zero: the padding of h, not of x)
          const float mean = bco[ci], scale = bco[C + ci], shift = bco[2 * C + ci];
          val.x = fmaxf((val.x - mean) * scale + shift, 0.f); val.y = fmaxf((val.y - mean) * scale + shift, 0.f);
          val.z = fmaxf((val.z - mean) * scale + shift, 0.f); val.w = fmaxf((val.w - mean) * scale + shift, 0.f);
          if (ry >= 1 && ry <= ROWS && ci / 16 == ct)
            *reinterpret_cast<float4*>(B->h + (((size_t)img * C + ci) * HW + gy) * HW + 4 * v) = val;
        }
      }
      *reinterpret_cast<float4*>(in_s + ci * G::CS + ry * G::WP + 4 + 4 * v) = val;
    };
    if (BNIN) {
      // the same two-phase staging with the BatchNorm's coefficients formed between the loads and the stores
      const float4* __restrict__ src = reinterpret_cast<const float4*>(w + (size_t)ct * 16 * G::K);
      float4 rw[(4 * G::K + 255) / 256], ri[(C * ROWSH * V / 2 + 255) / 256];
      fx::Totals ft;
      if (tid < C) ft = fx::load(B->fx, C, tid);           // first out: the coefficients are formed under the operand loads
      stage_load<4 * G::K, float4>(rw, [&](int i) { return src[i]; });
      stage_load<C * ROWSH * V / 2, float4>(ri, ld_in);
      if (tid < C) {
        double S, R;
        fx::finish(ft, S, R);
        const double mean_d = S / B->count;
        double var = R / B->count - mean_d * mean_d;
        if (var < 0.0) var = 0.0;
        const float invstd = (float)(1.0 / sqrt(var + B->eps));
        bco[tid] = (float)mean_d;
        bco[C + tid] = invstd * B->gamma[tid];
        bco[2 * C + tid] = B->beta[tid];
        if (ct == 0 && band == 0 && img == 0) {
          B->save_mean[tid] = (float)mean_d;
          B->save_invstd[tid] = invstd;
          const double unbiased = B->count > 1.0 ? var * (B->count / (B->count - 1.0)) : var;
          if (B->stat_log) {
            B->stat_log[2 * tid] = mean_d;
            B->stat_log[2 * tid + 1] = unbiased;
          } else if (B->running_mean) {
            B->running_mean[tid] = (float)((1.0 - B->momentum) * (double)B->running_mean[tid] + B->momentum * mean_d);
            B->running_var[tid] = (float)((1.0 - B->momentum) * (double)B->running_var[tid] + B->momentum * unbiased);
          }
        }
      }
      __syncthreads();
      stage_store<4 * G::K, float4>(rw, [&](int i, const float4& q) {
        w_s[slab_at(4 * i)] = q.x; w_s[slab_at(4 * i + 1)] = q.y;
        w_s[slab_at(4 * i + 2)] = q.z; w_s[slab_at(4 * i + 3)] = q.w;
      });
      stage_store<C * ROWSH * V / 2, float4>(ri, st_in);
    } else if (FRAG == FRAG_LDS) {
      const float4* __restrict__ src = reinterpret_cast<const float4*>(w + (size_t)ct * 16 * G::K);  // the tile's fragments
      stage2<4 * G::K, float4, C * ROWSH * V / 2, float4>(
          [&](int i) { return src[i]; },
          [&](int i, const float4& q) { *reinterpret_cast<float4*>(w_s + 4 * i) = q; },
          ld_in, st_in);
    } else if (FRAG == FRAG_REG) {
      const float4* __restrict__ src = reinterpret_cast<const float4*>(w + (size_t)ct * 16 * G::K) + lane;
#pragma unroll
      for (int f = 0; f < NF; ++f) fr[f] = src[f * 64];
      stage<C * ROWSH * V / 2, float4>(ld_in, st_in);
    } else if (!TRANSPOSE_W) {
      const float4* __restrict__ src = reinterpret_cast<const float4*>(w + (size_t)ct * 16 * G::K);  // contiguous
      stage2<4 * G::K, float4, C * ROWSH * V / 2, float4>(
          [&](int i) { return src[i]; },
          [&](int i, const float4& q) {
            w_s[slab_at(4 * i)] = q.x; w_s[slab_at(4 * i + 1)] = q.y;
            w_s[slab_at(4 * i + 2)] = q.z; w_s[slab_at(4 * i + 3)] = q.w;
          },
          ld_in, st_in);
    } else {
      // w'[n = ci_out][kidx = (co_in, r, s)] = w[co_in][ci_out][2-r][2-s]
      stage2<16 * G::K, float, C * ROWSH * V / 2, float4>(
          [&](int i) {
            const int n = i / G::K, kidx = i % G::K, co = kidx / 9, rs = kidx % 9;
            return w[((size_t)co * C + (ct * 16 + n)) * 9 + (8 - rs)];
          },
          [&](int i, float q) { w_s[slab_at(i)] = q; },
          ld_in, st_in);
    }
    for (int i = tid; i < C * ROWSH * 2; i += 256) {
      const int side = i & 1, ry = (i >> 1) % ROWSH, ci = (i >> 1) / ROWSH;
      in_s[ci * G::CS + ry * G::WP + (side ? HW + 4 : 3)] = 0.f;
    }
  }
  __syncthreads();
  SGMCMC_STAMP(1);
  // ---- K pipelined in two halves: the second half of the input channels is loaded (into registers) while the matrix
  // pipe works on the first half, stored to LDS and consumed after one more barrier -- a workgroup's MFMA phase no
  // longer waits for ALL of its operands (the two workgroups of a CU run their phases in lockstep, so nothing else
  // overlaps the staging latency)
  constexpr int V2 = HW / 4, ROWSH2 = ROWS + 2, H0 = C * ROWSH2 * V2 / 2;
  float4 r2[(H0 + 255) / 256];
  {
    const float* __restrict__ xi = x + (size_t)img * C * HW * HW;
    stage_load<H0, float4>(r2, [&](int j) {
      const int i = j + H0;
      const int v = i % V2, ry = (i / V2) % ROWSH2, ci = i / (V2 * ROWSH2);
      const int gy = y0 - 1 + ry;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gy >= 0 && gy < HW) val = *reinterpret_cast<const float4*>(xi + ((size_t)ci * HW + gy) * HW + 4 * v);
      return val;
    });
  }

  // ---- this wave's B operands: lane (n = lane & 15, k = lane >> 4) holds w_s[n][4*kk + k][rs]
  const int n = lane & 15, kq = lane >> 4;
  float breg[9][C / 4];
  if (FRAG) {
    constexpr int KS = C == 64 ? 2 : 1, KK = C / 4 / KS, QW4 = 9 * KK / 4;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const float4 q = FRAG == FRAG_REG ? fr[f] : *reinterpret_cast<const float4*>(w_s + (f * 64 + lane) * 4);
      const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int qi = 4 * (f % QW4) + j;
        breg[qi / KK][(f / QW4) * KK + qi % KK] = qv[j];
      }
    }
  } else {
#pragma unroll
    for (int rs = 0; rs < 9; ++rs)
#pragma unroll
      for (int kk = 0; kk < C / 4; ++kk) breg[rs][kk] = w_s[n * G::KP + (4 * kk + kq) * 9 + rs];
  }

  // ---- pixel tiles
  constexpr int NACC = G::PT_W == 1 ? 2 : G::PT_W;  // a single tile splits its K chain in two
  f32x4 acc[NACC];
  int abase[G::PT_W], orow[G::PT_W], ocol[G::PT_W];
#pragma unroll
  for (int t = 0; t < G::PT_W; ++t) {
    const int p = wave * G::PT_W + t;
    int yy, x0, m_y, m_x;
    if (HW >= 16) {
      constexpr int TPR = HW >= 16 ? HW / 16 : 1;                        // tiles per row
      yy = p / TPR; x0 = (p % TPR) * 16; m_y = 0; m_x = n;               // A row m = lane & 15
    } else {
      yy = 2 * p; x0 = 0; m_y = n >> 3; m_x = n & 7;                      // 2 rows of 8 pixels
    }
    abase[t] = kq * G::CS + (yy + m_y) * G::WP + x0 + m_x + 3;
    // D rows (pixels) 4*kq .. 4*kq+3 of this tile, column (channel) n
    const int m0 = 4 * kq;
    if (HW >= 16) { orow[t] = yy; ocol[t] = x0 + m0; }
    else { orow[t] = yy + (m0 >> 3); ocol[t] = m0 & 7; }
  }
  // the epilogue's own operands: issued before the MFMA loop, consumed after it
  float4 ex[G::PT_W], ey[G::PT_W], sy[G::PT_W], so[G::PT_W];
  float s_mean = 0.f, s_invstd = 0.f;
  if (EPI || SUMS) {
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
      const int go = group_offset(E, img, C);          // (scalar: folded into the base addresses)
      const float* __restrict__ gm = E->s_mean + go;
      const float* __restrict__ gi = E->s_invstd + go;
      s_mean = gm[ct * 16 + n]; s_invstd = gi[ct * 16 + n];
    }
  }
  // AFF: the lane's channel coefficients and its residual elements, requested before the MFMA loop like the others
  float v_mean = 0.f, v_invstd = 0.f, v_g = 0.f, v_b = 0.f;
  float4 vr[G::PT_W];
  if (AFF) {
    const int ch = ct * 16 + n;
    v_mean = V->mean[ch]; v_invstd = 1.0f / sqrtf(V->var[ch] + V->eps); v_g = V->gamma[ch]; v_b = V->beta[ch];
    if (V->residual) {
      const size_t cbase = ((size_t)img * C + ch) * HW * HW;
#pragma unroll
      for (int t = 0; t < G::PT_W; ++t)
        vr[t] = *reinterpret_cast<const float4*>(V->residual + cbase + (size_t)(y0 + orow[t]) * HW + ocol[t]);
    }
  }
#pragma unroll
  for (int a = 0; a < NACC; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  SGMCMC_STAMP(4);       // (operand fragments in registers: the first MFMA follows)
  float* __restrict__ yo = y + ((size_t)img * C + ct * 16 + n) * HW * HW;
  f32x4 vals[G::PT_W];
  float s1 = 0.f, z1 = 0.f, z2 = 0.f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    auto store_r2 = [&]() {
      stage_store<H0, float4>(r2, [&](int j, float4 val) {
        const int i = j + H0;
        const int v = i % V2, ry = (i / V2) % ROWSH2, ci = i / (V2 * ROWSH2);
        if (BNIN) {
          const int gy = y0 - 1 + ry;
          if (gy >= 0 && gy < HW) {
            const float mean = bco[ci], scale = bco[C + ci], shift = bco[2 * C + ci];
            val.x = fmaxf((val.x - mean) * scale + shift, 0.f); val.y = fmaxf((val.y - mean) * scale + shift, 0.f);
            val.z = fmaxf((val.z - mean) * scale + shift, 0.f); val.w = fmaxf((val.w - mean) * scale + shift, 0.f);
            if (ry >= 1 && ry <= ROWS && ci / 16 == ct)
              *reinterpret_cast<float4*>(B->h + (((size_t)img * C + ci) * HW + gy) * HW + 4 * v) = val;
          }
        }
        *reinterpret_cast<float4*>(in_s + ci * G::CS + ry * G::WP + 4 + 4 * v) = val;
      });
    };
    if (half == 1) {
      SGMCMC_STAMP(5);     // (the first half's MFMAs are issued)
      store_r2();
      __syncthreads();
      SGMCMC_STAMP(2);
    }
#pragma unroll
    for (int rs = 0; rs < 9; ++rs) {
      const int r = rs / 3, s = rs % 3;
#pragma unroll
      for (int k2 = 0; k2 < C / 8; ++k2) {
        const int kk = half * (C / 8) + k2;
#pragma unroll
        for (int t = 0; t < G::PT_W; ++t) {
          const float a = in_s[abase[t] + 4 * kk * G::CS + r * G::WP + s];
          const int ai = G::PT_W == 1 ? (kk & 1) : t;
          acc[ai] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, breg[rs][kk], acc[ai], 0, 0, 0);
        }
      }
    }
    if (half == 1) {
      // ---- store: lane holds 4 consecutive pixels of channel ct*16 + n
#pragma unroll
      for (int t = 0; t < G::PT_W; ++t) {
        f32x4 v = acc[t];
        if (G::PT_W == 1) v += acc[1];
        if (EPI) {
          v[0] += ey[t].x > 0.f ? ex[t].x : 0.f; v[1] += ey[t].y > 0.f ? ex[t].y : 0.f;
          v[2] += ey[t].z > 0.f ? ex[t].z : 0.f; v[3] += ey[t].w > 0.f ? ex[t].w : 0.f;
        }
        if (AFF) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = (v[j] - v_mean) * v_invstd * v_g + v_b;
          if (V->residual) { v[0] += vr[t].x; v[1] += vr[t].y; v[2] += vr[t].z; v[3] += vr[t].w; }
          if (V->relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
        }
        vals[t] = v;
        if (SUMS) {
          const float d0 = so[t].x > 0.f ? v[0] : 0.f, d1 = so[t].y > 0.f ? v[1] : 0.f;
          const float d2 = so[t].z > 0.f ? v[2] : 0.f, d3 = so[t].w > 0.f ? v[3] : 0.f;
          z1 += (d0 + d1) + (d2 + d3);
          z2 += (d0 * ((sy[t].x - s_mean) * s_invstd) + d1 * ((sy[t].y - s_mean) * s_invstd)) +
                (d2 * ((sy[t].z - s_mean) * s_invstd) + d3 * ((sy[t].w - s_mean) * s_invstd));
          if (E->mask_dx) v = f32x4{d0, d1, d2, d3};
        }
        sgmcmc_store4<(TRANSPOSE_W ? 64 : 1)>(y, yo + (size_t)(y0 + orow[t]) * HW + ocol[t], v[0], v[1], v[2], v[3]);
        if (STATS) s1 += (v[0] + v[1]) + (v[2] + v[3]);
      }
    }
  }
  SGMCMC_STAMP(3);
  if (SUMS) band_sums(z1, z2, lds, E->s_partial + ((size_t)(ct * 16) * E->n_slices + (img * G::BANDS + band)) * 2,
                      (size_t)E->n_slices * 2);
  if (STATS) {
    if (fx_out) band_stats_fx<G::PT_W>(vals, s1, ROWS * HW, lds, fx_out, C, ct * 16);
    else band_stats<G::PT_W>(vals, s1, ROWS * HW, lds, stats + ((size_t)(ct * 16) * n_slices + (img * G::BANDS + band)) * 2,
                             (size_t)n_slices * 2);
  }
  SGMCMC_STAMP(6);
}

template <int C, int HW, int ROWS, bool TRANSPOSE_W, bool STATS, int FRAG = 0>
__global__ __launch_bounds__(256) void conv3x3_kernel(const float* __restrict__ x,
                                                      const float* __restrict__ w,
                                                      float* __restrict__ y, double* __restrict__ stats,
                                                      int n_slices) {
  conv3x3_body<C, HW, ROWS, TRANSPOSE_W, STATS, false, false, false, false, FRAG>(
      xcd_remap<C>((int)blockIdx.x, (int)gridDim.x), x, w, y, stats, n_slices);
}

// the forward with its statistics on prepared fragments (`frag`: the convolution's forward fragments); FRAG_REG leaves
// the slab's share of the LDS unrequested
template <int C, int HW, int ROWS>
int launch_conv3x3_wfrag(const float* x, const float* frag, float* y, int n_img, double* stats, int form, hipStream_t s) {
  using G = Cfg<C, HW, ROWS>;
  const dim3 grid((unsigned)(n_img * G::BANDS * G::CT)), block(256);
  auto kl = conv3x3_kernel<C, HW, ROWS, false, true, FRAG_LDS>;
  auto kr = conv3x3_kernel<C, HW, ROWS, false, true, FRAG_REG>;
  constexpr size_t LDS_REG = G::LDS_BYTES - (size_t)16 * G::KP * sizeof(float);
  static_assert(LDS_REG >= 128 * sizeof(float), "band_stats reduces in the launch's LDS");
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kl), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)G::LDS_BYTES);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(kr), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_REG);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  const int n_slices = n_img * G::BANDS;
  if (form == FRAG_REG) SGMCMC_LAUNCH(kr, grid, block, LDS_REG, s, x, frag, y, stats, n_slices);
  else SGMCMC_LAUNCH(kl, grid, block, G::LDS_BYTES, s, x, frag, y, stats, n_slices);
  return (int)hipGetLastError();
}

template <int C, int HW, int ROWS>
__global__ __launch_bounds__(256) void conv3x3_eval_kernel(const float* __restrict__ x,
                                                                           const float* __restrict__ w,
                                                                           float* __restrict__ y, EvalBn V) {
  conv3x3_body<C, HW, ROWS, false, false, false, false, false, true>(xcd_remap<C>((int)blockIdx.x, (int)gridDim.x), x, w, y,
                                                                     nullptr, 0, nullptr, nullptr, nullptr, &V);
}

template <int C, int HW, int ROWS>
int launch_conv3x3_eval(const float* x, const float* w, float* y, int n_img, const EvalBn& V, hipStream_t s) {
  using G = Cfg<C, HW, ROWS>;
  auto k = conv3x3_eval_kernel<C, HW, ROWS>;
  static bool attr_done = false;
  if (!attr_done) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)G::LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  SGMCMC_LAUNCH(k, dim3((unsigned)(n_img * G::BANDS * G::CT)), dim3(256), G::LDS_BYTES, s, x, w, y, V);
  return (int)hipGetLastError();
}

template <int C, int HW, int ROWS>
int launch_conv3x3(const float* x, const float* w, float* y, int n_img, bool transpose_w, double* stats,
                   hipStream_t s) {
  using G = Cfg<C, HW, ROWS>;
  const dim3 grid((unsigned)(n_img * G::BANDS * G::CT)), block(256);
  auto kf = conv3x3_kernel<C, HW, ROWS, false, false>;
  auto ks = conv3x3_kernel<C, HW, ROWS, false, true>;
  auto kt = conv3x3_kernel<C, HW, ROWS, true, false>;
  static bool attr_done = false;
  if (!attr_done) {  // up to 160 KiB of LDS per workgroup on gfx950; above 64 KiB it has to be asked for
    for (const void* k : {reinterpret_cast<const void*>(kf), reinterpret_cast<const void*>(ks),
                          reinterpret_cast<const void*>(kt)}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  const int n_slices = n_img * G::BANDS;
  if (transpose_w) SGMCMC_LAUNCH(kt, grid, block, G::LDS_BYTES, s, x, w, y, nullptr, n_slices);
  else if (stats) SGMCMC_LAUNCH(ks, grid, block, G::LDS_BYTES, s, x, w, y, stats, n_slices);
  else SGMCMC_LAUNCH(kf, grid, block, G::LDS_BYTES, s, x, w, y, nullptr, n_slices);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- weight gradient
// dw[co,ci,r,s] = sum_{n,p} dy[n,co,p] x[n,ci,p+(r-1,s-1)]: GEMM with M = co, N = ci (per tap), K = pixels.
// One workgroup = 16 output channels x ITEMS (image, band) items; per item the x band (with halo)
// and the dy band are staged in LDS.  Wave (cit, ps) owns input-channel tile cit and a quarter /
// half / all of the band's pixels: per 4-pixel k-step ONE A fetch (dy) feeds the 9 taps' MFMAs,
// each with its own B fetch (shifted x) and its own accumulator tile.  The pixel splits are summed
// through LDS at the end and the workgroup writes ONE partial dw slab, TAP-MAJOR ([r,s][co][ci]: the 16 lanes
// of a tile row write 64 contiguous bytes; [co][ci][r,s] order scattered 4-byte stores 36 bytes apart and cost
// 4.5 us of the 64-channel launch); `wrw_reduce_kernel` adds the slabs in a fixed order (no atomics: the
// gradient is reproducible bit for bit) and transposes to [co][ci][r,s] on its one small write.
template <int C, int HW, int ROWS, bool ALIGNED16 = false>   // ALIGNED16: the round-2 strides (16-byte aligned rows: conv_fused_hip.inc)
struct WrwCfg {
  static constexpr int WP = HW + 8;
  static constexpr int CS_RAW = (ROWS + 2) * WP;
  // the 16 n-lanes of a B fetch index CHANNELS here, the 4 k-lanes consecutive pixels; ds_read_b32 serves lanes 0-31
  // (k-lanes 0, 1) and 32-63 in separate passes over 32 banks: stride = 2 mod 32 -> banks 2n + k, all distinct
  // (round 2 had 4 mod 64: channels n and n + 8 collided, every operand read of this kernel was 2-way conflicted).
  // 8-byte aligned only, so the staging stores are ds_write_b64 pairs (same LDS bandwidth as b128).
  static constexpr int CS = ALIGNED16 ? CS_RAW + ((4 - CS_RAW % 64) % 64 + 64) % 64 : CS_RAW + ((2 - CS_RAW % 32) % 32 + 32) % 32;
  static constexpr int NPIX = ROWS * HW;
  static constexpr int DS = NPIX + (ALIGNED16 ? 4 : 2);  // NPIX is a multiple of 64
  static constexpr int NCI = C / 16, PS = 4 / NCI;
  static constexpr int KSTEPS = NPIX / 4 / PS;  // per wave and item
  static constexpr int BANDS = HW / ROWS, CT = C / 16;
  // items per workgroup: fewer partial slabs at no MFMA cost.  64 channels: 4 (a slab is 147 KB there: 64 -> 32 slabs per
  // gradient, -24 MB of slab traffic per step: 1120 -> 1137 steps/s); with 4 at 32 channels the weight-gradient
  // workgroups become the launch's critical path (16.6 -> 20.0 us), so 2 elsewhere.
  static constexpr int ITEMS = C >= 64 ? 4 : 2;      // (A/B on one box, googleresnet steps/s at 16 / 32 channels: 1 -> 1,124, 2 -> 1,179, 4 -> 1,129)
  static constexpr int SLAB = 16 * C * 9;
  static constexpr int V = HW / 4, ROWSH = ROWS + 2;
  static constexpr int IN_V = C * ROWSH * V, NV = (IN_V + 255) / 256;      // float4 of an item's x band / dy band
  static constexpr int DY_V = 16 * NPIX / 4, NDV = (DY_V + 255) / 256;
  static constexpr size_t STAGE_FLOATS = (size_t)C * CS + 16 * DS, RED_FLOATS = 4 * 9 * 256;
  static constexpr size_t LDS_BYTES = (STAGE_FLOATS > RED_FLOATS ? STAGE_FLOATS : RED_FLOATS) * sizeof(float);
  static_assert(NPIX % 64 == 0 && 4 % NCI == 0, "tile geometry");
};

// Round 3: (1) the NEXT item's operands are loaded into registers while the matrix pipe works on the current one
// (a 64-channel workgroup walked its 4 items load -> MFMA -> load -> ...: 19 us of a launch whose data-gradient half
// needs 12); (2) the operands of k-step kk + 1 are fetched from LDS during the 9 MFMAs of k-step kk (the compiler's
// own schedule waited for every fetch right before its use: ~50 cycles per MFMA with one wave per SIMD);
// (3) conflict-free strides (WrwCfg).  Same items, same k order, same slabs: bit-identical results.
// MULT (a launch that carries several minibatches): the workgroup walks ITEMS x mult items, a RUN-TIME count -- its own
// instantiation, because with the compile-time count of the default the item loop is unrolled and scheduled across
// items (a run-time count in the one-minibatch launch cost 1.2 us per convolution gradient in the leapfrog step).
template <int C, int HW, int ROWS, bool MULT = false>
__device__ __forceinline__ void conv3x3_wrw_body(int b, const float* __restrict__ x,
                                                 const float* __restrict__ dy, float* __restrict__ part,
                                                 int n_items, int mult = 1) {
  using G = WrwCfg<C, HW, ROWS>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* __restrict__ in_s = lds;
  float* __restrict__ dy_s = lds + C * G::CS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = b % G::CT, pw = b / G::CT;
  const int cit = wave % G::NCI, ps = wave / G::NCI;
  const int n = lane & 15, kq = lane >> 4;

  auto load_item = [&](int item, float4 (&rx)[G::NV], float4 (&rd)[G::NDV]) {
    const int band = item % G::BANDS, img = item / G::BANDS;
    const int y0 = band * ROWS;
    const float* __restrict__ xi = x + (size_t)img * C * HW * HW;
    // dy band: 16 channels x NPIX contiguous pixels (rows y0 .. y0+ROWS-1 are contiguous in NCHW)
    const float* __restrict__ di = dy + (((size_t)img * C + ct * 16) * HW + y0) * HW;
#pragma unroll
    for (int it = 0; it < G::NV; ++it) {
      const int i = tid + it * 256;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((G::IN_V % 256 == 0) || i < G::IN_V) {
        const int v = i % G::V, ry = (i / G::V) % G::ROWSH, ci = i / (G::V * G::ROWSH);
        const int gy = y0 - 1 + ry;
        if (gy >= 0 && gy < HW) val = *reinterpret_cast<const float4*>(xi + ((size_t)ci * HW + gy) * HW + 4 * v);
      }
      rx[it] = val;
    }
#pragma unroll
    for (int it = 0; it < G::NDV; ++it) {
      const int i = tid + it * 256;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((G::DY_V % 256 == 0) || i < G::DY_V) {
        const int v = i % (G::NPIX / 4), co = i / (G::NPIX / 4);
        val = *reinterpret_cast<const float4*>(di + (size_t)co * HW * HW + 4 * v);
      }
      rd[it] = val;
    }
  };
  auto store_item = [&](const float4 (&rx)[G::NV], const float4 (&rd)[G::NDV]) {
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
  const int items = MULT ? G::ITEMS * mult : G::ITEMS;
  const int item0 = pw * items;
  SGMCMC_STAMP(0);
  SGMCMC_STAMP(7);
  if (item0 < n_items) load_item(item0, prx, prd);
  // halo columns (x = -1 and x = HW): zero once, the item stores only touch the interior
  for (int i = tid; i < C * G::ROWSH * 2; i += 256) {
    const int side = i & 1, ry = (i >> 1) % G::ROWSH, ci = (i >> 1) / G::ROWSH;
    in_s[ci * G::CS + ry * G::WP + (side ? HW + 4 : 3)] = 0.f;
  }
  const float* __restrict__ bsrc = in_s + (cit * 16 + n) * G::CS + kq + 3;
  const float* __restrict__ asrc = dy_s + n * G::DS + kq;

  for (int it = 0; it < items; ++it) {
    const int item = item0 + it;
    if (item >= n_items) break;
    if (it) __syncthreads();  // the previous item's operands are no longer being read
      store_item(prx, prd);
    __syncthreads();
    SGMCMC_STAMP(1 + 2 * (it & 1));
    if (it + 1 < items && item + 1 < n_items) load_item(item + 1, prx, prd);   // in flight during this item's MFMAs
    float a_cur, b_cur[9], a_nxt = 0.f, b_nxt[9];
    auto fetch = [&](int kk, float& a, float (&bv)[9]) {
      const int g = ps * G::KSTEPS + kk;             // 4-pixel group within the band
      const int row = g / (HW / 4), xg = g % (HW / 4);
      a = asrc[4 * g];
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) bv[rs] = bsrc[(row + rs / 3) * G::WP + 4 * xg + rs % 3];
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
    SGMCMC_STAMP(2 + 2 * (it & 1));
  }
  // ---- sum the pixel splits, write this workgroup's slab: part[pw][(ct*16 + co)][ci][rs]
  __syncthreads();
  float* __restrict__ red = lds;  // [wave][rs][256]
#pragma unroll
  for (int rs = 0; rs < 9; ++rs)
    *reinterpret_cast<float4*>(red + (wave * 9 + rs) * 256 + 4 * lane) =
        make_float4(acc[rs][0], acc[rs][1], acc[rs][2], acc[rs][3]);
  __syncthreads();
  float* __restrict__ out = part + (size_t)pw * (C * C * 9) + (size_t)ct * 16 * C;
  for (int i = tid; i < G::NCI * 9 * 256; i += 256) {
    const int e = i % 256, rs = (i / 256) % 9, ci_t = i / (256 * 9);
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < G::PS; ++q) v += red[((q * G::NCI + ci_t) * 9 + rs) * 256 + e];
    const int ln = e >> 2, vv = e & 3;               // D[row = 4*(ln>>4) + vv][col = ln & 15]
    const int co = 4 * (ln >> 4) + vv, ci = ci_t * 16 + (ln & 15);
    out[((size_t)rs * C + co) * C + ci] = v;       // tap-major slab: 16 consecutive ci per 64-byte run
  }
  SGMCMC_STAMP(6);
}

template <int C, int HW, int ROWS>
__global__ __launch_bounds__(256) void conv3x3_wrw_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ dy,
                                                          float* __restrict__ part, int n_items) {
  conv3x3_wrw_body<C, HW, ROWS>(xcd_remap<C>((int)blockIdx.x, (int)gridDim.x), x, dy, part, n_items);
}

// where element j of a slab lands in the output: slabs of `taps` > 1 are tap-major ([taps][E / taps]) and the
// output is tap-minor ([E / taps][taps], i.e. [co][ci][r,s])
__device__ __forceinline__ int slab_out_index(int j, int E, int taps) {
  if (taps <= 1) return j;
  const int inner = E / taps;
  return (j % inner) * taps + j / inner;
}

// out[slab_out_index(j)] = sum_{p < P} part[p*E + j], every element in a FIXED order that depends on (P, E) alone:
//   normal: a block = 64 elements x 4 slab groups; group q adds slabs q, q+4, ... (4 running sums, combined as
//           (b0 + b1) + (b2 + b3)); the 4 groups by a fixed tree;
//   wide  : many slabs of a small gradient (the first convolution's 896 slabs of 450 numbers): a block = 16 elements
//           x 16 slab groups, group q adds slabs q, q+16, ... the same way; the 16 groups by a fixed tree --
//           so that the serial chain per thread is P/16 long on E/16 blocks instead of P/4 on E/64.
__device__ __forceinline__ bool reduce_wide(int P, int E) { return P >= 256 && E <= 4096; }
// (round 3) vec: E a multiple of 4 and not `wide`: a block covers 256 elements -- a thread owns 4 consecutive ones and
// reads them as ONE 16-byte load per slab (1 KiB contiguous per slab and block instead of 256 B) -- with exactly the
// per-element order of the scalar block
__host__ __device__ __forceinline__ bool reduce_vec(int P, int E) { return !(P >= 256 && E <= 4096) && (E & 3) == 0; }
__host__ __device__ __forceinline__ int reduce_blocks(int P, int E) {
  return (P >= 256 && E <= 4096) ? (E + 15) / 16 : reduce_vec(P, E) ? (E + 255) / 256 : (E + 63) / 64;
}

// (sh: 4 KiB of the caller's LDS, 16-byte aligned.  DEEP: the loads in flight per round trip -- 32, or 8 for the rider
// workgroups of conv3x3_bwd_kernel, whose register budget belongs to the convolution roles; the additions are the same
// 4-at-a-time sequence either way: slab p + u * ng goes to running sum u % 4 in increasing u)
template <int DEEP = 32>
__device__ __forceinline__ void reduce_block_vec(const float* __restrict__ part, int P, int E, float* __restrict__ out,
                                                 int taps, int blk, float* __restrict__ sh) {
  float4* __restrict__ shv = reinterpret_cast<float4*>(sh);      // [4][64]
  const int le = threadIdx.x & 63, pg = threadIdx.x >> 6, ng = 4;
  const int e = (blk * 64 + le) * 4;
  const bool aligned = (reinterpret_cast<uintptr_t>(part) & 15) == 0;
  auto ld = [&](int p) {
    const float* __restrict__ src = part + (size_t)p * E + e;
    return aligned ? *reinterpret_cast<const float4*>(src) : make_float4(src[0], src[1], src[2], src[3]);
  };
  auto add = [](float4& acc, const float4& v) { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; };
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e < E) {
    float4 b0 = a, b1 = a, b2 = a, b3 = a;
    int p = pg;
    // a thread's slabs are a chain of round trips to memory: 32 (then 8) 16-byte loads in flight per trip, added in the
    // 4-at-a-time order whatever the batching (64 slabs per thread at 16 channels: 2 trips instead of 8)
    if constexpr (DEEP >= 32) for (; p + 31 * ng < P; p += 32 * ng) {
      float4 v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = ld(p + u * ng);
#pragma unroll
      for (int u = 0; u < 32; u += 4) { add(b0, v[u]); add(b1, v[u + 1]); add(b2, v[u + 2]); add(b3, v[u + 3]); }
    }
    for (; p + 7 * ng < P; p += 8 * ng) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ld(p + u * ng);
#pragma unroll
      for (int u = 0; u < 8; u += 4) { add(b0, v[u]); add(b1, v[u + 1]); add(b2, v[u + 2]); add(b3, v[u + 3]); }
    }
    for (; p + 3 * ng < P; p += 4 * ng) {
      const float4 v0 = ld(p), v1 = ld(p + ng), v2 = ld(p + 2 * ng), v3 = ld(p + 3 * ng);
      add(b0, v0); add(b1, v1); add(b2, v2); add(b3, v3);
    }
    for (; p < P; p += ng) add(b0, ld(p));
    a = make_float4((b0.x + b1.x) + (b2.x + b3.x), (b0.y + b1.y) + (b2.y + b3.y), (b0.z + b1.z) + (b2.z + b3.z),
                    (b0.w + b1.w) + (b2.w + b3.w));
  }
  shv[pg * 64 + le] = a;
  __syncthreads();
  if (pg == 0 && e < E) {
    const float4 q0 = shv[le], q1 = shv[64 + le], q2 = shv[128 + le], q3 = shv[192 + le];
    const float r[4] = {(q0.x + q1.x) + (q2.x + q3.x), (q0.y + q1.y) + (q2.y + q3.y), (q0.z + q1.z) + (q2.z + q3.z),
                        (q0.w + q1.w) + (q2.w + q3.w)};
#pragma unroll
    for (int j = 0; j < 4; ++j) out[slab_out_index(e + j, E, taps)] = r[j];
  }
}

constexpr int REDUCE_LDS_FLOATS = 1024;     // what reduce_block needs of its caller's LDS
template <int DEEP = 32>
__device__ __forceinline__ void reduce_block(const float* __restrict__ part, int P, int E, float* __restrict__ out,
                                             int taps, int blk, float* __restrict__ sh) {
  if (reduce_vec(P, E)) { reduce_block_vec<DEEP>(part, P, E, out, taps, blk, sh); return; }
  // sh as [16][16]; normal: [4][64] in the same storage
  const bool wide = reduce_wide(P, E);
  const int ew = wide ? 16 : 64, ng = wide ? 16 : 4;
  const int le = threadIdx.x % ew, pg = threadIdx.x / ew;
  const int e = blk * ew + le;
  float a = 0.f;
  if (e < E) {
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    int p = pg;
    for (; p + 15 * ng < P; p += 16 * ng) {     // 16 loads in flight per round trip, the same order of additions
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = part[(size_t)(p + u * ng) * E + e];
#pragma unroll
      for (int u = 0; u < 16; u += 4) { b0 += v[u]; b1 += v[u + 1]; b2 += v[u + 2]; b3 += v[u + 3]; }
    }
    for (; p + 3 * ng < P; p += 4 * ng) {
      b0 += part[(size_t)p * E + e];
      b1 += part[(size_t)(p + ng) * E + e];
      b2 += part[(size_t)(p + 2 * ng) * E + e];
      b3 += part[(size_t)(p + 3 * ng) * E + e];
    }
    for (; p < P; p += ng) b0 += part[(size_t)p * E + e];
    a = (b0 + b1) + (b2 + b3);
  }
  float* __restrict__ shf = sh;
  shf[pg * ew + le] = a;
  __syncthreads();
  if (pg == 0 && e < E) {
    float r;
    if (wide) {
      float q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        q[k] = (shf[(4 * k) * 16 + le] + shf[(4 * k + 1) * 16 + le]) + (shf[(4 * k + 2) * 16 + le] + shf[(4 * k + 3) * 16 + le]);
      r = (q[0] + q[1]) + (q[2] + q[3]);
    } else {
      r = (shf[le] + shf[64 + le]) + (shf[128 + le] + shf[192 + le]);
    }
    out[slab_out_index(e, E, taps)] = r;
  }
}

__global__ __launch_bounds__(256) void wrw_reduce_kernel(const float* __restrict__ part, int P, int E,
                                                         float* __restrict__ out, int taps) {
  __shared__ __attribute__((aligned(16))) float sh[REDUCE_LDS_FLOATS];
  reduce_block(part, P, E, out, taps, (int)blockIdx.x, sh);
}

// the same reduction for up to SGMCMC_REDUCE_JOBS weight gradients in one launch (the whole backward
// pass's slabs at once): block b belongs to the job whose block range contains it
struct ReduceJobs {
  sgmcmc_reduce_job job[SGMCMC_REDUCE_JOBS];
  int first_block[SGMCMC_REDUCE_JOBS + 1];
  int n;
};

__global__ __launch_bounds__(256) void wrw_reduce_many_kernel(ReduceJobs J) {
  __shared__ __attribute__((aligned(16))) float sh[REDUCE_LDS_FLOATS];
  int j = 0;
  while (j + 1 < J.n && (int)blockIdx.x >= J.first_block[j + 1]) ++j;
  // identical summation order to wrw_reduce_kernel: the result does not depend on the route
  reduce_block(J.job[j].part, J.job[j].n_slabs, J.job[j].numel, J.job[j].out, J.job[j].taps,
               (int)blockIdx.x - J.first_block[j], sh);
}

// Riders: up to SGMCMC_RIDE_JOBS slab reductions of EARLIER launches (reduce_block: the blocks of wrw_reduce_many_kernel,
// the same bits) as a third role of the merged backward launch.  Their slabs were complete when the launch that wrote
// them ended -- the kernel boundary is the only synchronisation -- and nothing but the sampler at the end of the pass
// reads their result, so they leave the dependent chain: a rider takes a workgroup slot that the first finished
// weight-gradient workgroups free and waits for memory while the data-gradient workgroups compute.
// first != 0: the riders lead the grid, padded to a multiple of 8 blocks so that the other roles keep their XCDs.
struct RideJobs {
  sgmcmc_reduce_job job[SGMCMC_RIDE_JOBS];
  int first_block[SGMCMC_RIDE_JOBS + 1];
  int n, first;
};
__host__ __device__ __forceinline__ int ride_blocks(const RideJobs& R) {
  return R.first ? (R.first_block[R.n] + 7) & ~7 : R.first_block[R.n];
}

// (Block order: the weight-gradient blocks come FIRST.  They process two items each and run about twice as
// long as a data-gradient block; dispatched first they overlap the data-gradient blocks instead of forming a
// half-empty tail round -- longest-processing-time-first over the 2 x 256 resident workgroup slots.)
// Both gradients of one convolution in ONE launch: n_dgrad blocks compute the data gradient
// (forward body on dy with transposed + flipped weights), the rest the weight-gradient slabs.  The two
// halves are independent, so they share the GPU instead of running back to back with a launch gap.
// (3 waves per SIMD = 3 workgroups per CU, what the LDS footprint admits: the ADD + SUMS variant at 16 channels sat two
// registers above that step.  At 64 channels the data gradient's 80 KB of LDS admit two workgroups per CU whatever is
// requested: asking for three only capped the registers at 168 and made the ADD + SUMS instantiation spill: two there)
// FRAG: the data-gradient role reads `w` as the convolution's prepared DATA-GRADIENT fragments (conv3x3_body, FRAG)
template <int C, int HW, int ROWS, bool EPI, bool SUMS, bool MULT = false, int FRAG = 0>
__global__ __launch_bounds__(256, (MULT || C >= 64) ? 2 : 3) void conv3x3_bwd_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ w,
                                                          const float* __restrict__ dy,
                                                          float* __restrict__ dx, float* __restrict__ part,
                                                          int n_dgrad, int n_items, BwdEpilogue E, RideJobs R) {
  const int n_ride = ride_blocks(R);
  const int n_wrw = (int)gridDim.x - n_dgrad - n_ride;
  int b = (int)blockIdx.x;
  if (n_ride) {      // (riders last: ids [n_wrw + n_dgrad, grid); first: ids [0, n_ride) -- the other roles' ids map as without)
    const int r = R.first ? b : b - (n_wrw + n_dgrad);
    if (R.first) b -= n_ride;
    if (r >= 0 && r < n_ride) {
      if (r >= R.first_block[R.n]) return;      // padding
      extern __shared__ __attribute__((aligned(16))) float lds[];
      int j = 0;
      while (j + 1 < R.n && r >= R.first_block[j + 1]) ++j;
      reduce_block<8>(R.job[j].part, R.job[j].n_slabs, R.job[j].numel, R.job[j].out, R.job[j].taps, r - R.first_block[j],
                      lds);
      return;
    }
  }
  // (both halves in image order per XCD: image i's weight-gradient items and its data-gradient tiles share dy in one L2)
  if (b < n_wrw) {
    conv3x3_wrw_body<C, HW, ROWS, MULT>(xcd_remap<C>(b, n_wrw), x, dy, part, n_items, E.wrw_mult);
  }
  else conv3x3_body<C, HW, ROWS, true, false, EPI, SUMS, false, false, FRAG>(xcd_remap<C>(b - n_wrw, n_dgrad), dy, w, dx,
                                                                             nullptr, 0, &E);
}

// ---- host-side pieces every convolution entry point shares -----------------------------------------------------
// The trunk's shape table, in ONE place: `return <expression>;` with constexpr C, HW, ROWS of (channels, hw), or the
// refusal (the caller keeps other shapes on the library path).
inline bool is_trunk_shape(int channels, int hw) {
  return (channels == 16 && hw == 32) || (channels == 32 && hw == 16) || (channels == 64 && hw == 8);
}
#define SGMCMC_FOR_TRUNK_SHAPE(channels, hw, ...)                                                                     \
  do {                                                                                                                \
    if ((channels) == 16 && (hw) == 32) { constexpr int C = 16, HW = 32, ROWS = 8; (void)ROWS; return __VA_ARGS__; } \
    if ((channels) == 32 && (hw) == 16) { constexpr int C = 32, HW = 16, ROWS = 8; (void)ROWS; return __VA_ARGS__; } \
    if ((channels) == 64 && (hw) == 8) { constexpr int C = 64, HW = 8, ROWS = 8; (void)ROWS; return __VA_ARGS__; }   \
    return (int)hipErrorInvalidValue;                                                                                 \
  } while (0)

// The tail of every launch that left P partial slabs per gradient: the caller takes the count and has them summed
// later (sgmcmc_wrw_reduce_many, a carrier launch's riders), or each set is summed here by one wrw_reduce_kernel
// launch, in the order given -- same kernel, same grid either way, so the route does not show in the bits.
struct SlabSet {
  const float* part;   // [P][E]
  int E;
  float* out;          // nullptr: this gradient was not asked for
  int taps;            // sgmcmc_reduce_job.taps
};
inline int finish_slabs(int* deferred_slabs, int P, hipStream_t s, const SlabSet* sets, int n_sets) {
  if (deferred_slabs) {
    *deferred_slabs = P;
  } else {
    for (const SlabSet* q = sets; q != sets + n_sets; ++q)
      if (q->out)
        SGMCMC_LAUNCH(wrw_reduce_kernel, dim3((unsigned)reduce_blocks(P, q->E)), dim3(256), 0, s, q->part, P, q->E, q->out,
                      q->taps);
  }
  return (int)hipGetLastError();
}
inline int finish_slabs(int* deferred_slabs, int P, hipStream_t s, std::initializer_list<SlabSet> sets) {
  return finish_slabs(deferred_slabs, P, s, sets.begin(), (int)sets.size());
}

// sgmcmc_conv_bwd_epilogue -> BwdEpilogue, with every check any entry point makes (n_slices is the launcher's).  An
// entry that supports only part of the epilogue adds its own refusals; wrw_mult is read by sgmcmc_conv3x3_bwd_ex alone.
inline int epilogue_from_abi(const sgmcmc_conv_bwd_epilogue* epi, int n_img, BwdEpilogue& E) {
  E = BwdEpilogue{};
  if (epi->e_out && !epi->e_dout) return (int)hipErrorInvalidValue;      // (e_dout alone: added unmasked)
  const bool sums = epi->s_partial != nullptr;
  if (sums && (!epi->s_y || !epi->s_out || !epi->s_mean || !epi->s_invstd)) return (int)hipErrorInvalidValue;
  if (epi->mask_dx && !sums) return (int)hipErrorInvalidValue;
  if (epi->wrw_mult < 0 || epi->wrw_mult > 64) return (int)hipErrorInvalidValue;
  E.e_dout = epi->e_dout; E.e_out = epi->e_out;
  E.mask_dx = epi->mask_dx != 0;
  E.wrw_mult = epi->wrw_mult;
  if (sums) {
    E.s_y = epi->s_y; E.s_out = epi->s_out; E.s_mean = epi->s_mean; E.s_invstd = epi->s_invstd;
    E.s_partial = epi->s_partial;
    if (epi->group_imgs < 0 || (epi->group_imgs > 0 && n_img % epi->group_imgs)) return (int)hipErrorInvalidValue;
    set_groups(E, epi->group_imgs);
  }
  return 0;
}

template <int C, int HW, int ROWS>
int launch_wrw(const float* x, const float* dy, float* dw, float* part, int n_img, hipStream_t s) {
  using G = WrwCfg<C, HW, ROWS>;
  const int n_items = n_img * G::BANDS, P = (n_items + G::ITEMS - 1) / G::ITEMS;
  auto k = conv3x3_wrw_kernel<C, HW, ROWS>;
  static bool attr_done = false;
  if (!attr_done) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  SGMCMC_LAUNCH(k, dim3((unsigned)(P * G::CT)), dim3(256), G::LDS_BYTES, s, x, dy, part, n_items);
  const int E = C * C * 9;
  SGMCMC_LAUNCH(wrw_reduce_kernel, dim3((unsigned)reduce_blocks(P, E)), dim3(256), 0, s, part, P, E, dw, 9);
  return (int)hipGetLastError();
}

template <int C, int HW, int ROWS>
// which: 0 = both gradients in one launch; 1 = the data-gradient workgroups only; 2 = the weight-gradient workgroups
// only -- the two halves are independent, so a caller may also put them on two streams: the weight gradient then
// leaves the backward pass's critical path (sgmcmc_conv3x3_bwd_part, a measured alternative)
int launch_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* part, int n_img,
               int* n_slabs, hipStream_t s, const BwdEpilogue& E = BwdEpilogue{}, int which = 0,
               const RideJobs& R = RideJobs{}) {
  using G = WrwCfg<C, HW, ROWS>;
  using F = Cfg<C, HW, ROWS>;
  const int mult = (E.wrw_mult > 1 && E.s_partial != nullptr) ? E.wrw_mult : 1;
  const int n_items = n_img * G::BANDS, P = (n_items + G::ITEMS * mult - 1) / (G::ITEMS * mult);
  const int n_dgrad = which == 2 ? 0 : n_img * F::BANDS * F::CT;
  const int n_wrw = which == 1 ? 0 : P * G::CT;
  const size_t lds = F::LDS_BYTES > G::LDS_BYTES ? F::LDS_BYTES : G::LDS_BYTES;
  auto k00 = conv3x3_bwd_kernel<C, HW, ROWS, false, false>;
  auto k10 = conv3x3_bwd_kernel<C, HW, ROWS, true, false>;
  auto k01 = conv3x3_bwd_kernel<C, HW, ROWS, false, true>;
  auto k11 = conv3x3_bwd_kernel<C, HW, ROWS, true, true>;
  auto m01 = conv3x3_bwd_kernel<C, HW, ROWS, false, true, true>;      // (grouped launches come with the sums epilogue)
  auto m11 = conv3x3_bwd_kernel<C, HW, ROWS, true, true, true>;
  static bool attr_done = false;
  if (!attr_done) {
    for (const void* f : {reinterpret_cast<const void*>(k00), reinterpret_cast<const void*>(k10),
                          reinterpret_cast<const void*>(k01), reinterpret_cast<const void*>(k11),
                          reinterpret_cast<const void*>(m01), reinterpret_cast<const void*>(m11)}) {
      const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  BwdEpilogue Ev = E;
  Ev.n_slices = n_img * F::BANDS;
  Ev.wrw_mult = mult;
  static_assert(F::LDS_BYTES >= REDUCE_LDS_FLOATS * sizeof(float), "the riders reduce in the launch's LDS");
  const dim3 grid((unsigned)(n_dgrad + n_wrw + ride_blocks(R)));
  const bool epi = E.e_dout != nullptr, sums = E.s_partial != nullptr;
  if (mult > 1 && epi) SGMCMC_LAUNCH(m11, grid, dim3(256), lds, s, x, w, dy, dx, part, n_dgrad, n_items, Ev, R);
  else if (mult > 1) SGMCMC_LAUNCH(m01, grid, dim3(256), lds, s, x, w, dy, dx, part, n_dgrad, n_items, Ev, R);
  else if (epi && sums) SGMCMC_LAUNCH(k11, grid, dim3(256), lds, s, x, w, dy, dx, part, n_dgrad, n_items, Ev, R);
  else if (epi) SGMCMC_LAUNCH(k10, grid, dim3(256), lds, s, x, w, dy, dx, part, n_dgrad, n_items, Ev, R);
  else if (sums) SGMCMC_LAUNCH(k01, grid, dim3(256), lds, s, x, w, dy, dx, part, n_dgrad, n_items, Ev, R);
  else SGMCMC_LAUNCH(k00, grid, dim3(256), lds, s, x, w, dy, dx, part, n_dgrad, n_items, Ev, R);
  if (which == 1) return (int)hipGetLastError();        // no slabs were written
  return finish_slabs(n_slabs, P, s, {{part, C * C * 9, dw, 9}});
}

// launch_bwd's merged launch with the data-gradient role on prepared fragments, for what the leapfrog step runs: the
// sums epilogue (with or without the shortcut's add), one minibatch, with or without riders; the slabs are always left
// to the caller (*n_slabs) or reduced here, as launch_bwd does
template <int C, int HW, int ROWS>
int launch_bwd_wfrag(const float* x, const float* frag, const float* dy, float* dx, float* dw, float* part, int n_img,
                     int* n_slabs, hipStream_t s, const BwdEpilogue& E, const RideJobs& R, int form) {
  using G = WrwCfg<C, HW, ROWS>;
  using F = Cfg<C, HW, ROWS>;
  const int n_items = n_img * G::BANDS, P = (n_items + G::ITEMS - 1) / G::ITEMS;
  const int n_dgrad = n_img * F::BANDS * F::CT, n_wrw = P * G::CT;
  const size_t lds = F::LDS_BYTES > G::LDS_BYTES ? F::LDS_BYTES : G::LDS_BYTES;
  auto l01 = conv3x3_bwd_kernel<C, HW, ROWS, false, true, false, FRAG_LDS>;
  auto l11 = conv3x3_bwd_kernel<C, HW, ROWS, true, true, false, FRAG_LDS>;
  auto r01 = conv3x3_bwd_kernel<C, HW, ROWS, false, true, false, FRAG_REG>;
  auto r11 = conv3x3_bwd_kernel<C, HW, ROWS, true, true, false, FRAG_REG>;
  static bool attr_done = false;
  if (!attr_done) {
    for (const void* f : {reinterpret_cast<const void*>(l01), reinterpret_cast<const void*>(l11),
                          reinterpret_cast<const void*>(r01), reinterpret_cast<const void*>(r11)}) {
      const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  BwdEpilogue Ev = E;
  Ev.n_slices = n_img * F::BANDS;
  Ev.wrw_mult = 1;
  const dim3 grid((unsigned)(n_dgrad + n_wrw + ride_blocks(R)));
  const bool epi = E.e_dout != nullptr, reg = form == FRAG_REG;
  auto k = epi ? (reg ? r11 : l11) : (reg ? r01 : l01);
  SGMCMC_LAUNCH(k, grid, dim3(256), lds, s, x, frag, dy, dx, part, n_dgrad, n_items, Ev, R);
  return finish_slabs(n_slabs, P, s, {{part, C * C * 9, dw, 9}});
}

}  // namespace conv

// data gradient AND weight gradient of the convolution in one launch (+ the slab reduction)
extern "C" int sgmcmc_conv3x3_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw,
                                  float* scratch, int n_img, int channels, int hw, int* deferred_slabs,
                                  void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !dy || !dx || !scratch || n_img <= 0 || (!dw && !deferred_slabs))
    return (int)hipErrorInvalidValue;
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_bwd<C, HW, ROWS>(x, w, dy, dx, dw, scratch, n_img, deferred_slabs,
                                                                     (hipStream_t)stream));
}

static int conv3x3_bwd_with(const float* x, const float* w, const float* dy, float* dx, float* dw, float* scratch,
                            int n_img, int channels, int hw, int* d, hipStream_t s, const conv::BwdEpilogue& E,
                            int which = 0, const conv::RideJobs& R = conv::RideJobs{}) {
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_bwd<C, HW, ROWS>(x, w, dy, dx, dw, scratch, n_img, d, s, E, which, R));
}

extern "C" int sgmcmc_conv3x3_bwd_add(const float* x, const float* w, const float* dy, float* dx, const float* e_dout,
                                      const float* e_out, float* dw, float* scratch, int n_img, int channels, int hw,
                                      int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !dy || !dx || !e_dout || !e_out || !scratch || n_img <= 0 || (!dw && !deferred_slabs))
    return (int)hipErrorInvalidValue;
  conv::BwdEpilogue E{};
  E.e_dout = e_dout; E.e_out = e_out;
  return conv3x3_bwd_with(x, w, dy, dx, dw, scratch, n_img, channels, hw, deferred_slabs, (hipStream_t)stream, E);
}

static int conv3x3_bwd_ex_with(const float* x, const float* w, const float* dy, float* dx,
                               const sgmcmc_conv_bwd_epilogue* epi, float* dw, float* scratch, int n_img, int channels,
                               int hw, int* deferred_slabs, void* stream, const conv::RideJobs& R) {
  if (!x || !w || !dy || !dx || !epi || !scratch || n_img <= 0 || (!dw && !deferred_slabs))
    return (int)hipErrorInvalidValue;
  conv::BwdEpilogue E;
  if (const int bad = conv::epilogue_from_abi(epi, n_img, E)) return bad;
  return conv3x3_bwd_with(x, w, dy, dx, dw, scratch, n_img, channels, hw, deferred_slabs, (hipStream_t)stream, E, 0, R);
}

extern "C" int sgmcmc_conv3x3_bwd_ex(const float* x, const float* w, const float* dy, float* dx,
                                     const sgmcmc_conv_bwd_epilogue* epi, float* dw, float* scratch, int n_img,
                                     int channels, int hw, int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  return conv3x3_bwd_ex_with(x, w, dy, dx, epi, dw, scratch, n_img, channels, hw, deferred_slabs, stream, conv::RideJobs{});
}

// sgmcmc_reduce_job[n_jobs] -> conv::RideJobs, with the checks of every entry point that takes riders
static int riders_from_abi(const sgmcmc_reduce_job* jobs, int n_jobs, int riders_first, conv::RideJobs& R) {
  if (n_jobs < 0 || n_jobs > SGMCMC_RIDE_JOBS || (n_jobs && !jobs)) return (int)hipErrorInvalidValue;
  R = conv::RideJobs{};
  R.n = n_jobs;
  R.first = riders_first != 0;
  int blocks = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const sgmcmc_reduce_job& q = jobs[j];
    if (!q.part || !q.out || q.n_slabs <= 0 || q.numel <= 0 || (q.taps > 1 && q.numel % q.taps)) return (int)hipErrorInvalidValue;
    R.job[j] = q;
    R.first_block[j] = blocks;
    blocks += conv::reduce_blocks(q.n_slabs, q.numel);
  }
  R.first_block[n_jobs] = blocks;
  return 0;
}

// ... with up to SGMCMC_RIDE_JOBS slab reductions of earlier launches riding in the grid (conv::RideJobs)
extern "C" int sgmcmc_conv3x3_bwd_ride(const float* x, const float* w, const float* dy, float* dx,
                                       const sgmcmc_conv_bwd_epilogue* epi, float* dw, float* scratch, int n_img,
                                       int channels, int hw, int* deferred_slabs, const sgmcmc_reduce_job* jobs,
                                       int n_jobs, int riders_first, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  conv::RideJobs R{};
  if (const int bad = riders_from_abi(jobs, n_jobs, riders_first, R)) return bad;
  return conv3x3_bwd_ex_with(x, w, dy, dx, epi, dw, scratch, n_img, channels, hw, deferred_slabs, stream, R);
}

// ---- the same forward and merged backward launches on PREPARED weight fragments (conv3x3_body, FRAG) ------------------
static int wfrag_form(int form) { return form == 1 ? conv::FRAG_LDS : form == 2 ? conv::FRAG_REG : 0; }

extern "C" int sgmcmc_conv3x3_wfrag_fwd(const float* x, const float* frag_fwd, float* y, int n_img, int channels, int hw,
                                        double* stats, int form, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const int f = wfrag_form(form);
  if (!x || !frag_fwd || !y || !stats || n_img <= 0 || !f) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_conv3x3_wfrag<C, HW, ROWS>(x, frag_fwd, y, n_img, stats, f, s));
}

static int conv3x3_wfrag_bwd_with(const float* x, const float* frag, const float* dy, float* dx, float* dw, float* scratch,
                                  int n_img, int channels, int hw, int* d, hipStream_t s, const conv::BwdEpilogue& E,
                                  const conv::RideJobs& R, int form) {
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_bwd_wfrag<C, HW, ROWS>(x, frag, dy, dx, dw, scratch, n_img, d, s, E, R, form));
}

extern "C" int sgmcmc_conv3x3_wfrag_bwd(const float* x, const float* frag_dgrad, const float* dy, float* dx,
                                        const sgmcmc_conv_bwd_epilogue* epi, float* dw, float* scratch, int n_img,
                                        int channels, int hw, int* deferred_slabs, const sgmcmc_reduce_job* jobs,
                                        int n_jobs, int riders_first, int form, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  const int f = wfrag_form(form);
  if (!x || !frag_dgrad || !dy || !dx || !epi || !scratch || n_img <= 0 || (!dw && !deferred_slabs) || !f)
    return (int)hipErrorInvalidValue;
  conv::BwdEpilogue E;
  if (const int bad = conv::epilogue_from_abi(epi, n_img, E)) return bad;
  if (!E.s_partial || E.wrw_mult > 1) return (int)hipErrorInvalidValue;      // the step's variants only (sgmcmc_hip.h)
  conv::RideJobs R{};
  if (const int bad = riders_from_abi(jobs, n_jobs, riders_first, R)) return bad;
  return conv3x3_wfrag_bwd_with(x, frag_dgrad, dy, dx, dw, scratch, n_img, channels, hw, deferred_slabs, (hipStream_t)stream,
                                E, R, f);
}

#ifdef SGMCMC_STAMPS
extern "C" int sgmcmc_debug_stamps(unsigned long long* host_dst, int n_blocks) {
  return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(conv::g_stamps), (size_t)n_blocks * 8 * sizeof(unsigned long long));
}
#endif

extern "C" int sgmcmc_wrw_reduce_many(const sgmcmc_reduce_job* jobs, int n_jobs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!jobs || n_jobs <= 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  for (int base = 0; base < n_jobs; base += SGMCMC_REDUCE_JOBS) {
    conv::ReduceJobs J;
    J.n = n_jobs - base < SGMCMC_REDUCE_JOBS ? n_jobs - base : SGMCMC_REDUCE_JOBS;
    int blocks = 0;
    for (int j = 0; j < J.n; ++j) {
      const sgmcmc_reduce_job& q = jobs[base + j];
      if (!q.part || !q.out || q.n_slabs <= 0 || q.numel <= 0 || (q.taps > 1 && q.numel % q.taps)) return (int)hipErrorInvalidValue;
      J.job[j] = q;
      J.first_block[j] = blocks;
      blocks += conv::reduce_blocks(q.n_slabs, q.numel);
    }
    J.first_block[J.n] = blocks;
    SGMCMC_LAUNCH(conv::wrw_reduce_many_kernel, dim3((unsigned)blocks), dim3(256), 0, s, J);
  }
  return (int)hipGetLastError();
}

extern "C" int64_t sgmcmc_conv3x3_wrw_scratch_floats(int n_img, int channels, int hw) {
  const int rows = 8;
  if (!conv::is_trunk_shape(channels, hw) || n_img <= 0) return -1;
  const int n_items = n_img * (hw / rows);
  const int per = channels >= 64 ? 4 : 2;   // items per slab (WrwCfg::ITEMS)
  return (int64_t)((n_items + per - 1) / per) * channels * channels * 9;
}

extern "C" int sgmcmc_conv3x3_wrw(const float* x, const float* dy, float* dw, float* scratch, int n_img,
                                  int channels, int hw, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !dy || !dw || !scratch || n_img <= 0) return (int)hipErrorInvalidValue;
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_wrw<C, HW, ROWS>(x, dy, dw, scratch, n_img, (hipStream_t)stream));
}

extern "C" int sgmcmc_conv3x3_stat_slices(int n_img, int channels, int hw) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!conv::is_trunk_shape(channels, hw) || n_img <= 0) return -1;
  return n_img * (hw / 8);
}

extern "C" int sgmcmc_conv3x3_bn_eval(const float* x, const float* w, const float* gamma, const float* beta,
                                      const float* running_mean, const float* running_var, double eps,
                                      const float* residual, int relu, float* y, int n_img, int channels, int hw,
                                      void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !gamma || !beta || !running_mean || !running_var || !y || n_img <= 0) return (int)hipErrorInvalidValue;
  const conv::EvalBn V = {gamma, beta, running_mean, running_var, residual, (float)eps, relu};
  hipStream_t s = (hipStream_t)stream;
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_conv3x3_eval<C, HW, ROWS>(x, w, y, n_img, V, s));
}

extern "C" int sgmcmc_conv3x3(const float* x, const float* w, float* y, int n_img, int channels, int hw,
                              int transpose_w, double* stats, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !y || n_img <= 0 || (stats && transpose_w)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const bool t = transpose_w != 0;
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_conv3x3<C, HW, ROWS>(x, w, y, n_img, t, stats, s));
}
