// MEASURED ALTERNATIVES of conv_hip.inc, compiled with -DSGMCMC_ALTERNATIVES only (include/sgmcmc_hip_alternatives.h):
// the forward whose statistics go to fx slots and its consumer with the BatchNorm + ReLU folded into the operand staging
// (conv3x3_body<..., BNIN>), and the two halves of the merged backward launch as separate launches (side stream).
namespace conv {

// forward whose batch statistics go to fx slots (the consumer: conv3x3_bnin_kernel)
template <int C, int HW, int ROWS>
__global__ __launch_bounds__(256) void conv3x3_fx_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         float* __restrict__ y, long long* __restrict__ fx_out) {
  conv3x3_body<C, HW, ROWS, false, true>(xcd_remap<C>((int)blockIdx.x, (int)gridDim.x), x, w, y, nullptr, 0, nullptr, fx_out);
}
// forward on relu(BatchNorm(x)) formed while staging (BnIn), statistics of its own output per slice as conv3x3_kernel
template <int C, int HW, int ROWS>
__global__ __launch_bounds__(256) void conv3x3_bnin_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           float* __restrict__ y, double* __restrict__ stats,
                                                           int n_slices, BnIn B) {
  conv3x3_body<C, HW, ROWS, false, true, false, false, true>(xcd_remap<C>((int)blockIdx.x, (int)gridDim.x), x, w, y, stats,
                                                             n_slices, nullptr, nullptr, &B);
}

template <int C, int HW, int ROWS>
int launch_conv3x3_fold(const float* x, const float* w, float* y, int n_img, long long* fx_out, double* stats,
                        const BnIn* B, hipStream_t s) {
  using G = Cfg<C, HW, ROWS>;
  const dim3 grid((unsigned)(n_img * G::BANDS * G::CT)), block(256);
  auto kx = conv3x3_fx_kernel<C, HW, ROWS>;
  auto kb = conv3x3_bnin_kernel<C, HW, ROWS>;
  constexpr size_t LDS_B = G::LDS_BYTES + 3 * C * sizeof(float);
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kx), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(kb), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_B);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  if (B) SGMCMC_LAUNCH(kb, grid, block, LDS_B, s, x, w, y, stats, n_img * G::BANDS, *B);
  else SGMCMC_LAUNCH(kx, grid, block, G::LDS_BYTES, s, x, w, y, fx_out);
  return (int)hipGetLastError();
}

}  // namespace conv

extern "C" int sgmcmc_conv3x3_bwd_part(const float* x, const float* w, const float* dy, float* dx,
                                       const sgmcmc_conv_bwd_epilogue* epi, float* scratch, int n_img, int channels,
                                       int hw, int which, int* deferred_slabs, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (which != 1 && which != 2) return (int)hipErrorInvalidValue;
  if (!dy || n_img <= 0) return (int)hipErrorInvalidValue;
  conv::BwdEpilogue E{};
  if (which == 1) {            // data gradient (+ epilogues)
    if (!w || !dx) return (int)hipErrorInvalidValue;
    if (epi) {
      if (const int bad = conv::epilogue_from_abi(epi, n_img, E)) return bad;
      E.wrw_mult = 0;          // (this half writes no slabs)
    }
  } else if (!x || !scratch || !deferred_slabs) {       // weight-gradient slabs: always left for sgmcmc_wrw_reduce_many
    return (int)hipErrorInvalidValue;
  }
  return conv3x3_bwd_with(x, w, dy, dx, nullptr, scratch, n_img, channels, hw, deferred_slabs, (hipStream_t)stream, E, which);
}

extern "C" int64_t sgmcmc_fx_slot_int64(int channels) {
  return channels <= 0 ? -1 : (int64_t)conv::fx::SLOTS * conv::fx::LIMBS * channels * conv::fx::LINE;
}

/* forward; the batch statistics of y (sum, sum of squares per channel) are ADDED to fx (zeroed by the caller) */
extern "C" int sgmcmc_conv3x3_fx(const float* x, const float* w, float* y, int n_img, int channels, int hw,
                                 int64_t* fx, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !y || !fx || n_img <= 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  long long* f = reinterpret_cast<long long*>(fx);
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_conv3x3_fold<C, HW, ROWS>(x, w, y, n_img, f, nullptr, nullptr, s));
}

/* y = conv3x3(relu(BatchNorm(x)), w): the BatchNorm (training mode, batch statistics from bn->fx as left by
 * sgmcmc_conv3x3_fx) and the ReLU applied while the operands are staged; bn->h <- relu(BatchNorm(x)) as a side output;
 * stats as sgmcmc_conv3x3 (required) */
extern "C" int sgmcmc_conv3x3_bnin(const float* x, const float* w, float* y, int n_img, int channels, int hw,
                                   double* stats, const sgmcmc_bn_in* bn, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!x || !w || !y || !stats || n_img <= 0 || !bn || !bn->fx || !bn->gamma || !bn->beta || !bn->save_mean ||
      !bn->save_invstd || !bn->h || (bn->running_mean == nullptr) != (bn->running_var == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const conv::BnIn B = {reinterpret_cast<const long long*>(bn->fx), bn->gamma, bn->beta, bn->save_mean, bn->save_invstd,
                        bn->running_mean, bn->running_var, bn->stat_log, bn->momentum, bn->eps,
                        (double)n_img * hw * hw, bn->h};
  SGMCMC_FOR_TRUNK_SHAPE(channels, hw, conv::launch_conv3x3_fold<C, HW, ROWS>(x, w, y, n_img, nullptr, stats, &B, s));
}

