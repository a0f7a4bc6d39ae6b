// MEASURED ALTERNATIVE (include/sgmcmc_hip_alternatives.h: sgmcmc_conv3x3_bwd_uniform), not in the shipped library.
// In the googleresnet step (profiles/r06_ab_uniform_backward.txt): 16.7-16.95 us per launch against 17.2-17.55 us for the
// merged two-role launch, but twice the weight-gradient slabs at 32 channels (one per (image, band)) -- the pass's slab
// reduction 16.8 -> 21.4 us: GPU busy 796.0 -> 793.8 us, 1,242.5 vs 1,244.2 steps/s.  A wash; the text below says why.
//
// UNIFORM backward convolution at 16 @ 32x32 and 32 @ 16x16 (round 6): ONE kind of workgroup computes the data gradient
// AND the weight-gradient slab of its (image, band) items from ONE staging of the operands.  Reference: the gradient of
// R1 (inference.py:215-223) through the stride-1 convolutions of models/google_resnet.py:34-43.
//
// Why: conv::conv3x3_bwd_kernel runs two ROLES in one launch -- data-gradient workgroups (forward body on dy) and
// weight-gradient workgroups -- and the launch takes the SUM of the two roles' times (profiles/r05_backward_timeline.txt:
// 8.9 + 10.3 -> 17-19 us at 16 @ 32x32): each role is a serial chain load -> LDS -> MFMA -> store, and the second role's
// operands reach LDS only when the first one's waves leave the matrix pipe.  Here a wave carries 288 MFMAs (144 of the
// data gradient, 144 of the weight gradient) behind ONE operand staging; the dx stores of the first half leave under
// the MFMAs of the second.
// What the lab's in-kernel stamps showed (tools/conv_lab/lab_uni.hip): a workgroup lives 13.3 us -- operands in LDS 1.3 us,
// the three MFMA phases 2.6 + 1.9 + 4.2 us (the pipe alone: 7.7 us for 2 x 288 MFMAs per SIMD), three barriers 2.6 us of
// wave skew, slab reduction 1.1 us -- plus 2.8 us of dispatch ramp and drain.  The merged launch keeps three independent
// workgroups per CU whose phases drift apart; eight waves behind common barriers do not, and what the single staging saves
// (40 KB of loads per CU) the lock-step gives back.  Three things that each cost 1-2 us until fixed are kept as comments
// where they bit: a branch around a load (vmcnt(0)), 30 loads per thread issued up front (the address path blocks the
// wave), epilogue arithmetic hoisted to its loads (pin()).
//
// Workgroup = 8 waves (512 threads), one per CU, 256 per launch at batch 128:
//   16 channels: two TEAMS of 4 waves, one (image, band of 8 rows) item each; the weight slab staged once for both
//   32 channels: one item; wave (ct, w4) owns output-channel tile ct of the data gradient
// LDS per item: the dy band WITH halo, all C channels (the data gradient contracts over them), the x band WITHOUT halo
// (below), the transposed + flipped weight slab.
//
//   data gradient    dx[ci,p]      = sum_{co,r,s} dy[co, p-(r-1,s-1)] w[co,ci,r,s]       M = 16 pixels, N = 16 ci, K = (co, tap)
//                    = conv::conv3x3_body<TRANSPOSE_W>: the same MFMA order per accumulator, the same epilogue -> THE SAME BITS
//   weight gradient  dw[co,ci,r,s] = sum_q dy[co, q-(r-1,s-1)] x[ci,q]                   M = 16 co, N = 16 ci, K = 4 pixels q
//                    summed over the band's OWN pixels q of x (conv::conv3x3_wrw_body sums over the band's pixels of dy
//                    and reads x with a halo): every (p, q) pair of the image is still counted once, by the band that owns
//                    q -- so the halo band that the data gradient needs anyway (dy) is the shifted operand of the 9 taps
//                    and x is staged without halo.  One slab per workgroup, tap-major, summed by wrw_reduce_many as before.
//
// dy is read two ways: by the data gradient with the 16 m-lanes on consecutive PIXELS and the 4 k-lanes on channels
// 4kk .. 4kk+3 (conflict free when channels c, c+1 start 16 banks apart), and by the weight gradient with the 16 lanes on
// CHANNELS and the k-lanes on consecutive pixels (conflict free when the 16 channels of a tile start on distinct even
// banks).  One layout serves both: channel c of a tile starts at bank g(c) = 2 (c >> 1) + 16 (c & 1): pairs 16 apart, the
// sixteen starts {0, 16, 2, 18, ..., 14, 30} all even and distinct.  Channel pitch S0 = 0 mod 32 (+ 32 per 16-channel tile).

#ifndef CONVU_STAMP
#define CONVU_STAMP(k)      /* lab builds (tools/conv_lab/lab_uni.hip -DUNI_STAMPS): wall-clock stamps of a workgroup's phases */
#endif

namespace convu {

using conv::f32x4;
using conv::BwdEpilogue;

template <int C, int HW>
struct Cfg {
  static constexpr int ROWS = 8, ROWSH = ROWS + 2;
  static constexpr int WP = HW + 8;                       // row pitch: 4 pad | W interior | 4 pad (halo at 3 and W+4)
  static constexpr int CS_RAW = ROWSH * WP;
  static constexpr int S0 = ((CS_RAW + 14 + 31) / 32) * 32;   // (g(c+1) - g(c) >= -14 inside a tile)
  static constexpr int CT = C / 16;
  static constexpr int TEAMS = C == 16 ? 2 : 1;           // items per workgroup
  static constexpr int TT = 512 / TEAMS;                  // threads per team
  static constexpr int DY_FLOATS = C * S0 + 32 * CT + 32;
  static constexpr int NPIX = ROWS * HW, XS = NPIX + 2;   // x channel pitch = 2 mod 32: the 16 ci lanes on distinct even banks
  static constexpr int X_FLOATS = C * XS;
  static constexpr int K = 9 * C, KP = K + ((2 - K % 32) % 32 + 32) % 32;
  static constexpr int W_FLOATS = C * KP;                 // [ct][16][KP]
  static constexpr int BANDS = HW / ROWS;
  static constexpr int PT = ROWS * HW / 16, PT_W = PT / 4;    // pixel tiles per item / per wave of its 4
  static constexpr int V = HW / 4;
  static constexpr int NDY = C * ROWSH * V, NX = C * ROWS * V, NW = C * C * 9 / 4;   // float4 per item / per item / per workgroup
  static constexpr int IDY = (NDY + TT - 1) / TT, IX = (NX + TT - 1) / TT, IW = (NW + 511) / 512;
  static constexpr int NCI = C / 16;                      // ci tiles
  static constexpr int PS = 8 / TEAMS / (CT * NCI);       // pixel splits of an item's weight gradient: 4 (16 ch), 2 (32 ch)
  static constexpr int KSTEPS = NPIX / 4 / PS;            // 16 either way
  static constexpr int STAGE_FLOATS = TEAMS * (DY_FLOATS + X_FLOATS) + W_FLOATS;
  static constexpr int RED_FLOATS = 8 * 9 * 256;
  static constexpr int SUMS_AT = STAGE_FLOATS > RED_FLOATS ? STAGE_FLOATS : RED_FLOATS;
  static constexpr size_t LDS_BYTES = (size_t)(SUMS_AT + 2 * 2 * 4 * 16) * sizeof(float);
  static_assert(HW >= 16 && PT % 4 == 0 && KSTEPS * PS * 4 == NPIX, "tile geometry");
};

// The value is "produced" HERE as far as the compiler can tell: arithmetic on a loaded operand cannot be hoisted above this
// point -- without it the epilogue's compares and subtractions were placed right behind their loads, in the middle of the
// data gradient's MFMA loop, with an s_waitcnt vmcnt(0) in front of them.
__device__ __forceinline__ void pin(float4& q) { asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w)); }

// where channel c of the dy band starts (floats)
template <int S0>
__device__ __forceinline__ int dy_base(int c) { return c * S0 + 2 * ((c >> 1) & 7) + 16 * (c & 1) + 32 * (c >> 4); }

// EPI: 0 none; 1 dx += e_dout * [e_out > 0]; 2 dx += e_dout (it arrives masked: its producer ran with mask_dx).  A template
// parameter, not a run-time test of e_out: a branch around a load makes the compiler wait for EVERY load in flight there.
template <int C, int HW, int EPI, bool SUMS>
__global__ __launch_bounds__(512, 2) void bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ dy, float* __restrict__ dx,
                                                     float* __restrict__ part, BwdEpilogue E) {
  using G = Cfg<C, HW>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = wave >> 2, w4 = wave & 3;
  const int pw = conv::xcd_remap<C>((int)blockIdx.x, (int)gridDim.x);
  const int team = G::TEAMS == 2 ? grp : 0;
  const int ttid = G::TEAMS == 2 ? (tid & 255) : tid;
  const int item = pw * G::TEAMS + team;
  const int band = item % G::BANDS, img = item / G::BANDS, y0 = band * G::ROWS;
  const int ct = G::CT == 2 ? grp : 0;                     // data gradient: this wave's tile of dx channels
  float* __restrict__ dy_s = lds + team * G::DY_FLOATS;
  float* __restrict__ x_s = lds + G::TEAMS * G::DY_FLOATS + team * G::X_FLOATS;
  float* __restrict__ w_s = lds + G::TEAMS * (G::DY_FLOATS + G::X_FLOATS);
  float* __restrict__ sums_s = lds + G::SUMS_AT;           // [grp][quantity][w4][16], never overlaid
  const int n = lane & 15, kq = lane >> 4;
  CONVU_STAMP(0);

  // ---- Loads.  A CU's vector-memory path moves ~11-16 bytes per cycle and holds a bounded number of requests: a wave that
  // issues more than that BLOCKS until earlier ones return.  With a thread's 20-30 loads issued up front, the first operands
  // reached LDS 2.5-4 us late and the first MFMA phase grew by 2 us (lab stamps) -- so only what the first two phases
  // need is requested here,
  //   A  w[co < C/2], dy channels < C/2      -> first K half of the data gradient
  //   B  w[co >= C/2], dy channels >= C/2    -> second K half
  // and the rest -- X: the x band, D: the epilogue's operands, tile by tile -- one or two at a time BETWEEN THE TAPS of the
  // data gradient's MFMA loop (`issue_slot`).  Every load is unconditional (clamped index, halo rows zeroed when stored):
  // behind a branch the compiler cannot count what is in flight and waits for everything.
  constexpr int HDY = G::NDY / 2, HW_ = G::NW / 2;
  constexpr int IDYH = (HDY + G::TT - 1) / G::TT, IWH = (HW_ + 511) / 512;
  float4 rdy[2][IDYH], rx[G::IX], rw[2][IWH];
  int wdst[2][IWH][4], ddst[2][IDYH], xdst[G::IX];
  bool dzero[2][IDYH];
  const float* __restrict__ dyi = dy + (size_t)img * C * HW * HW;
  const float* __restrict__ xi = x + (size_t)img * C * HW * HW;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int it = 0; it < IWH; ++it) {
      const int i = min(tid + it * 512, HW_ - 1);
      rw[h][it] = reinterpret_cast<const float4*>(w)[h * HW_ + i];
    }
#pragma unroll
    for (int it = 0; it < IDYH; ++it) {
      const int i = h * HDY + min(ttid + it * G::TT, HDY - 1);
      const int v = i % G::V, ry = (i / G::V) % G::ROWSH, c = i / (G::V * G::ROWSH);
      const int gy = y0 - 1 + ry, gyc = min(max(gy, 0), HW - 1);
      rdy[h][it] = *reinterpret_cast<const float4*>(dyi + ((size_t)c * HW + gyc) * HW + 4 * v);
      dzero[h][it] = gy != gyc;
      ddst[h][it] = dy_base<G::S0>(c) + ry * G::WP + 4 + 4 * v;
    }
  }
  // Where everything goes in LDS, computed NOW (under the latency of the loads): the scatter of the weight slab is a dozen
  // integer divisions per element -- 0.9 us of VALU work per store phase, matrix pipe idle, when it sat between the wait
  // and the stores (lab stamps).
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int it = 0; it < IWH; ++it) {
      const int i = tid + it * 512;
      // w'[ct][n = ci & 15][co * 9 + (8 - rs)] = w[co][ci][rs]: the forward body's slab of the transposed + flipped weights
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = 4 * (h * HW_ + i) + j, rs = e % 9, ci = (e / 9) % C, co = e / (9 * C);
        wdst[h][it][j] = (ci >> 4) * 16 * G::KP + (ci & 15) * G::KP + co * 9 + 8 - rs;
      }
    }
#pragma unroll
  for (int it = 0; it < G::IX; ++it) {
    const int i = ttid + it * G::TT;
    const int v = i % G::V, ry = (i / G::V) % G::ROWS, c = i / (G::V * G::ROWS);
    xdst[it] = c * G::XS + ry * HW + 4 * v;
  }
  static_assert(G::NX % G::TT == 0, "x band: whole iterations");
  // ---- the data gradient's tiles (conv::conv3x3_body's assignment: wave w4 of the item's four, tiles w4 PT_W + t)
  int abase[G::PT_W], orow[G::PT_W], ocol[G::PT_W];
#pragma unroll
  for (int t = 0; t < G::PT_W; ++t) {
    const int p = w4 * G::PT_W + t;
    constexpr int TPR = HW / 16;
    const int yy = p / TPR, x0 = (p % TPR) * 16;
    abase[t] = kq * G::S0 + 2 * (kq >> 1) + 16 * (kq & 1) + yy * G::WP + x0 + n + 3;
    orow[t] = yy; ocol[t] = x0 + 4 * kq;
  }
  for (int i = ttid; i < C * G::ROWSH * 2; i += G::TT) {
    const int side = i & 1, ry = (i >> 1) % G::ROWSH, c = (i >> 1) / G::ROWSH;
    dy_s[dy_base<G::S0>(c) + ry * G::WP + (side ? HW + 4 : 3)] = 0.f;
  }
  // a K half's operands into LDS
  auto store_half = [&](int h) {
#pragma unroll
    for (int it = 0; it < IWH; ++it) {
      const int i = tid + it * 512;
      if ((HW_ % 512 == 0) || i < HW_) {
        w_s[wdst[h][it][0]] = rw[h][it].x; w_s[wdst[h][it][1]] = rw[h][it].y;
        w_s[wdst[h][it][2]] = rw[h][it].z; w_s[wdst[h][it][3]] = rw[h][it].w;
      }
    }
#pragma unroll
    for (int it = 0; it < IDYH; ++it) {
      const int j = ttid + it * G::TT;
      if ((HDY % G::TT == 0) || j < HDY) {
        float4 q = rdy[h][it];
        if (dzero[h][it]) q = make_float4(0.f, 0.f, 0.f, 0.f);
        float2* d = reinterpret_cast<float2*>(dy_s + ddst[h][it]);
        d[0] = make_float2(q.x, q.y); d[1] = make_float2(q.z, q.w);
      }
    }
  };
  // the later phases' loads, dealt to the SLOTS between the data gradient's taps
  float4 ex[G::PT_W], ey[G::PT_W], sy[G::PT_W], so[G::PT_W];
  float s_mean = 0.f, s_invstd = 0.f;
  constexpr int NE = (EPI == 1 ? 2 : EPI == 2 ? 1 : 0) + (SUMS ? 2 : 0);      // epilogue loads per tile
  constexpr int NLATE = G::IX + G::PT_W * NE, PER = (NLATE + 17) / 18;
#ifndef CONVU_MID_STORE
#define CONVU_MID_STORE 6
#endif
  constexpr int MID_STORE = CONVU_MID_STORE;      // tap after which the next phase's operands are stored (8: at the phase's end)
  const size_t ebase = ((size_t)img * C + ct * 16 + n) * HW * HW;
  auto issue_one = [&](int q) {
    if (q < G::IX) {
      const int i = ttid + q * G::TT;
      const int v = i % G::V, ry = (i / G::V) % G::ROWS, c = i / (G::V * G::ROWS);
      rx[q] = *reinterpret_cast<const float4*>(xi + ((size_t)c * HW + y0 + ry) * HW + 4 * v);
    } else if (q < NLATE) {
      constexpr int NE1 = NE > 0 ? NE : 1;
      const int t = (q - G::IX) / NE1;
      int k = (q - G::IX) % NE1;
      const size_t off = ebase + (size_t)(y0 + orow[t]) * HW + ocol[t];
      if (EPI != 0) { if (k == 0) ex[t] = *reinterpret_cast<const float4*>(E.e_dout + off); --k; }
      if (EPI == 1) { if (k == 0) ey[t] = *reinterpret_cast<const float4*>(E.e_out + off); --k; }
      if (SUMS) {
        if (k == 0) sy[t] = *reinterpret_cast<const float4*>(E.s_y + off);
        if (k == 1) so[t] = *reinterpret_cast<const float4*>(E.s_out + off);
      }
    }
  };
  auto issue_slot = [&](int slot) {
#pragma unroll
    for (int j = 0; j < PER; ++j) issue_one(slot * PER + j);
  };
  if (SUMS) {
    const int go = conv::group_offset(&E, img, C);
    s_mean = E.s_mean[go + ct * 16 + n]; s_invstd = E.s_invstd[go + ct * 16 + n];
  }
  store_half(0);
  __syncthreads();
  CONVU_STAMP(1);

  // ================================================================ data gradient: 144 MFMAs in two K halves
  // (the order of conv3x3_body: input-channel halves, then taps, then the half's k-steps -- every accumulator sees its
  //  products in that kernel's order: the same bits)
  f32x4 dacc[G::PT_W];
#pragma unroll
  for (int t = 0; t < G::PT_W; ++t) dacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (half == 1) {
      CONVU_STAMP(2);
      __syncthreads();
      CONVU_STAMP(3);
    }
    float breg[9][C / 8];
    const float* __restrict__ wt = w_s + ct * 16 * G::KP + n * G::KP + kq * 9 + 36 * half * (C / 8);
#pragma unroll
    for (int rs = 0; rs < 9; ++rs)
#pragma unroll
      for (int k2 = 0; k2 < C / 8; ++k2) breg[rs][k2] = wt[36 * k2 + rs];
#pragma unroll
    for (int rs = 0; rs < 9; ++rs) {
      const int r = rs / 3, s = rs % 3;
#pragma unroll
      for (int k2 = 0; k2 < C / 8; ++k2) {
        const int kk = half * (C / 8) + k2;
        const int koff = 4 * kk * G::S0 + 2 * ((2 * kk) & 7) + 32 * (kk >> 2);     // dy_base(4 kk + kq) - its kq part
#pragma unroll
        for (int t = 0; t < G::PT_W; ++t) {
          const float a = dy_s[abase[t] + koff + r * G::WP + s];
          dacc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, breg[rs][k2], dacc[t], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      issue_slot(half * 9 + rs);
      // The NEXT phase's operands go to LDS from inside this one (their loads were issued a phase earlier and have landed;
      // the regions they go to are not read before the next barrier): the store phases between the barriers, in which
      // every wave of the CU stored and the matrix pipe idled, took 0.65 + 0.45 us (lab stamps).
      if (half == 0 && rs == MID_STORE) store_half(1);
      if (half == 1 && rs == MID_STORE) {
#pragma unroll
        for (int it = 0; it < G::IX; ++it) {
          float2* d = reinterpret_cast<float2*>(x_s + xdst[it]);
          d[0] = make_float2(rx[it].x, rx[it].y); d[1] = make_float2(rx[it].z, rx[it].w);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  CONVU_STAMP(4);
  __syncthreads();
  CONVU_STAMP(5);

  // ================================================================ weight gradient: 144 MFMAs in PT_W parts; after part t
  // the data gradient's tile t gets its epilogue (its operands were requested last and arrive about now) and leaves --
  // the stores drain under the next part's MFMAs
  f32x4 acc[9];
#pragma unroll
  for (int rs = 0; rs < 9; ++rs) acc[rs] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    // wave -> (co tile, ci tile, pixel split) of its item
    const int cot = G::CT == 2 ? grp : 0, cit = G::CT == 2 ? (w4 & 1) : 0, ps = G::CT == 2 ? (w4 >> 1) : w4;
    const float* __restrict__ asrc = dy_s + dy_base<G::S0>(cot * 16 + n) + kq + 5 + 2 * G::WP;   // tap (r, s): - r WP - s
    const float* __restrict__ bsrc = x_s + (cit * 16 + n) * G::XS + kq;
    float a_cur[9], b_cur, a_nxt[9], b_nxt = 0.f;
    auto fetch = [&](int kk, float (&av)[9], float& bv) {
      const int g = ps * G::KSTEPS + kk;               // 4-pixel group of the band
      const int row = g / G::V, xg = g % G::V;
      bv = bsrc[4 * g];
#pragma unroll
      for (int rs = 0; rs < 9; ++rs) av[rs] = asrc[(row - rs / 3) * G::WP + 4 * xg - rs % 3];
    };
    float* __restrict__ yo = dx + ebase;
    float z1 = 0.f, z2 = 0.f;
    fetch(0, a_cur, b_cur);
    constexpr int KPART = G::KSTEPS / G::PT_W;
#pragma unroll
    for (int t = 0; t < G::PT_W; ++t) {
#pragma unroll
      for (int k2 = 0; k2 < KPART; ++k2) {
        const int kk = t * KPART + k2;
        if (kk + 1 < G::KSTEPS) fetch(kk + 1, a_nxt, b_nxt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rs = 0; rs < 9; ++rs) acc[rs] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[rs], b_cur, acc[rs], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        b_cur = b_nxt;
#pragma unroll
        for (int rs = 0; rs < 9; ++rs) a_cur[rs] = a_nxt[rs];
      }
      // ---- epilogue of the data gradient's tile t: lane holds 4 consecutive pixels of channel ct * 16 + n
      f32x4 v = dacc[t];
      if (EPI != 0) pin(ex[t]);
      if (EPI == 1) pin(ey[t]);
      if (SUMS) { pin(sy[t]); pin(so[t]); }
      if (EPI == 1) {
        v[0] += ey[t].x > 0.f ? ex[t].x : 0.f; v[1] += ey[t].y > 0.f ? ex[t].y : 0.f;
        v[2] += ey[t].z > 0.f ? ex[t].z : 0.f; v[3] += ey[t].w > 0.f ? ex[t].w : 0.f;
      } else if (EPI == 2) {
        v[0] += ex[t].x; v[1] += ex[t].y; v[2] += ex[t].z; v[3] += ex[t].w;
      }
      if (SUMS) {
        const float d0 = so[t].x > 0.f ? v[0] : 0.f, d1 = so[t].y > 0.f ? v[1] : 0.f;
        const float d2 = so[t].z > 0.f ? v[2] : 0.f, d3 = so[t].w > 0.f ? v[3] : 0.f;
        z1 += (d0 + d1) + (d2 + d3);
        z2 += (d0 * ((sy[t].x - s_mean) * s_invstd) + d1 * ((sy[t].y - s_mean) * s_invstd)) +
              (d2 * ((sy[t].z - s_mean) * s_invstd) + d3 * ((sy[t].w - s_mean) * s_invstd));
        if (E.mask_dx) v = f32x4{d0, d1, d2, d3};
      }
      sgmcmc_store4<64>(dx, yo + (size_t)(y0 + orow[t]) * HW + ocol[t], v[0], v[1], v[2], v[3]);
    }
    if (SUMS) {      // conv::band_sums' tree: lanes n, n+16, n+32, n+48, then the item's 4 waves in order (below)
      z1 += __shfl_xor(z1, 16, 64); z1 += __shfl_xor(z1, 32, 64);
      z2 += __shfl_xor(z2, 16, 64); z2 += __shfl_xor(z2, 32, 64);
      if (lane < 16) { sums_s[((grp * 2 + 0) * 4 + w4) * 16 + lane] = z1; sums_s[((grp * 2 + 1) * 4 + w4) * 16 + lane] = z2; }
    }
  }
  // ---- the waves' partial tiles through LDS (over the operands: everybody is done with them), ONE slab per workgroup
  CONVU_STAMP(6);
  __syncthreads();
  CONVU_STAMP(7);
  float* __restrict__ red = lds;      // [wave][rs][256]
#pragma unroll
  for (int rs = 0; rs < 9; ++rs)
    *reinterpret_cast<float4*>(red + (wave * 9 + rs) * 256 + 4 * lane) = make_float4(acc[rs][0], acc[rs][1], acc[rs][2], acc[rs][3]);
  if (SUMS && (tid & 255) < 16) {
    const int c = tid & 15, g2 = tid >> 8;            // grp = team (16 channels) / channel tile (32 channels)
    const int it2 = pw * G::TEAMS + (G::TEAMS == 2 ? g2 : 0), ct2 = G::CT == 2 ? g2 : 0;
    const float* __restrict__ q1 = sums_s + (g2 * 2 + 0) * 64 + c;
    const float* __restrict__ q2 = sums_s + (g2 * 2 + 1) * 64 + c;
    double* __restrict__ dst = E.s_partial + ((size_t)(ct2 * 16 + c) * E.n_slices + it2) * 2;
    dst[0] = ((double)q1[0] + (double)q1[16]) + ((double)q1[32] + (double)q1[48]);
    dst[1] = ((double)q2[0] + (double)q2[16]) + ((double)q2[32] + (double)q2[48]);
  }
  __syncthreads();
  // thread -> (tile, tap, lane ln of the tile's D layout): the lane's float4 (rows co = 4 (ln >> 4) + {0..3}, column ci =
  // ln & 15) of every wave that holds a partial of this tile by ONE ds_read_b128 each; the four sums leave as dword stores,
  // 16 consecutive lanes writing 64 contiguous bytes.  Fixed order of additions: ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).
  float* __restrict__ out = part + (size_t)pw * (C * C * 9);
  for (int i = tid; i < G::CT * G::NCI * 9 * 64; i += 512) {
    const int ln = i & 63, rs = (i >> 6) % 9, tile = i / (9 * 64), cot = G::CT == 2 ? tile >> 1 : 0, cit = G::CT == 2 ? tile & 1 : 0;
    float4 r;
    if (G::CT == 1) {
      float4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const float4*>(red + (q * 9 + rs) * 256 + 4 * ln);
      r.x = ((v[0].x + v[1].x) + (v[2].x + v[3].x)) + ((v[4].x + v[5].x) + (v[6].x + v[7].x));
      r.y = ((v[0].y + v[1].y) + (v[2].y + v[3].y)) + ((v[4].y + v[5].y) + (v[6].y + v[7].y));
      r.z = ((v[0].z + v[1].z) + (v[2].z + v[3].z)) + ((v[4].z + v[5].z) + (v[6].z + v[7].z));
      r.w = ((v[0].w + v[1].w) + (v[2].w + v[3].w)) + ((v[4].w + v[5].w) + (v[6].w + v[7].w));
    } else {      // wave = cot * 4 + (ps * 2 + cit)
      const float4 a = *reinterpret_cast<const float4*>(red + ((cot * 4 + cit) * 9 + rs) * 256 + 4 * ln);
      const float4 b = *reinterpret_cast<const float4*>(red + ((cot * 4 + 2 + cit) * 9 + rs) * 256 + 4 * ln);
      r = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    float* __restrict__ o = out + ((size_t)rs * C + cot * 16 + 4 * (ln >> 4)) * C + cit * 16 + (ln & 15);
    o[0] = r.x; o[C] = r.y; o[2 * C] = r.z; o[3 * C] = r.w;
  }
  CONVU_STAMP(8);
}

template <int C, int HW>
int n_slabs(int n_img) { return n_img * Cfg<C, HW>::BANDS / Cfg<C, HW>::TEAMS; }

// the whole backward of one convolution: data gradient (+ epilogue) and P = n_slabs slabs of the weight gradient
template <int C, int HW>
int launch(const float* x, const float* w, const float* dy, float* dx, float* part, int n_img, hipStream_t s,
           const BwdEpilogue& E) {
  using G = Cfg<C, HW>;
  auto k00 = bwd_kernel<C, HW, 0, false>;
  auto k10 = bwd_kernel<C, HW, 1, false>;
  auto k20 = bwd_kernel<C, HW, 2, false>;
  auto k01 = bwd_kernel<C, HW, 0, true>;
  auto k11 = bwd_kernel<C, HW, 1, true>;
  auto k21 = bwd_kernel<C, HW, 2, true>;
  static bool attr_done = false;
  if (!attr_done) {
    for (const void* f : {reinterpret_cast<const void*>(k00), reinterpret_cast<const void*>(k10),
                          reinterpret_cast<const void*>(k20), reinterpret_cast<const void*>(k01),
                          reinterpret_cast<const void*>(k11), reinterpret_cast<const void*>(k21)}) {
      const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  BwdEpilogue Ev = E;
  Ev.n_slices = n_img * G::BANDS;
  const dim3 grid((unsigned)n_slabs<C, HW>(n_img));
  const int epi = E.e_dout == nullptr ? 0 : E.e_out != nullptr ? 1 : 2;
  const bool sums = E.s_partial != nullptr;
  auto k = sums ? (epi == 0 ? k01 : epi == 1 ? k11 : k21) : (epi == 0 ? k00 : epi == 1 ? k10 : k20);
  SGMCMC_LAUNCH(k, grid, dim3(512), G::LDS_BYTES, s, x, w, dy, dx, part, Ev);
  return (int)hipGetLastError();
}

}  // namespace convu

extern "C" int sgmcmc_conv3x3_bwd_uniform_slabs(int n_img, int channels, int hw) {
  if (n_img <= 0) return -1;
  if (channels == 16 && hw == 32) return convu::n_slabs<16, 32>(n_img);
  if (channels == 32 && hw == 16) return convu::n_slabs<32, 16>(n_img);
  return -1;
}

extern "C" int sgmcmc_conv3x3_bwd_uniform(const float* x, const float* w, const float* dy, float* dx,
                                          const sgmcmc_conv_bwd_epilogue* epi, float* scratch, int n_img, int channels,
                                          int hw, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !dy || !dx || !scratch || n_img <= 0) return (int)hipErrorInvalidValue;
  conv::BwdEpilogue E{};
  if (epi) {
    if (epi->wrw_mult > 1 || epi->group_imgs != 0) return (int)hipErrorInvalidValue;      // (no groups on this route)
    if (const int bad = conv::epilogue_from_abi(epi, n_img, E)) return bad;
  }
  hipStream_t s = (hipStream_t)stream;
  if (channels == 16 && hw == 32) return convu::launch<16, 32>(x, w, dy, dx, scratch, n_img, s, E);
  if (channels == 32 && hw == 16) return convu::launch<32, 16>(x, w, dy, dx, scratch, n_img, s, E);
  return (int)hipErrorInvalidValue;
}
