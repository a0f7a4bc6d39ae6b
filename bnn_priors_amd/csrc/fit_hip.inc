// Fitting the data-driven priors to stacks of weight samples (fp64, deterministic; definitions in include/sgmcmc_hip.h,
// restated in tests/prior_fit_reference.py).  The stack [S, *shape] is read in place through its strides: a GEOMETRY
// (sgmcmc_fit_geometry) names the events, the F vectors of an event and the P positions of a vector.  Kernels:
//
//   pass_kernel<T, false>  moments: one pass with a shift taken from the data (the median of three vectors per position)
//                          over sum d, sum d d^T, sum d^3, sum d^4 per workgroup
//   pass_kernel<T, true>   kernel A of the multivariate-t EM: per event M and u, then sum u, A, B and the two log sums
//   moments_kernel         one workgroup: adds the workgroups' partials in ascending order, central moments
//   mvt_init_kernel        theta_0 from the moments
//   mvt_update_kernel      kernel B: one workgroup adds the partials; its first thread forms mu, S, the Cholesky and
//                          inverse factor, solves Liu & Rubin's equation for nu and applies the stopping rule
//   abs_kernel             sums of |d|, log|d|, |d|^beta (log|d|)^k at a given location and beta (element-wise families)
//
// A tile of rows (vectors) is staged in LDS as d = x - shift in fp64, loaded in the order of the stack's memory; then a
// thread owns one accumulated entry -- (a, b) of B, a of A, a scalar -- and one slice of the tile's rows, since no lane
// can hold the P (P + 1) / 2 = 325 entries of B.  Tile and grid are functions of (events, P, F) alone; every sum runs in
// an order fixed by them.  No atomics, no allocation, no host round trip.

namespace fit {

constexpr int kMaxP = SGMCMC_FILTER_MAX_P;
constexpr int kThreads = 256;
constexpr int kTileDoubles = SGMCMC_FIT_TILE_DOUBLES;   // the staged d of one tile
constexpr int kMaxRows = SGMCMC_FIT_TILE_ROWS;          // rows (vectors), hence events, of one tile
constexpr int kMaxBlocks = SGMCMC_FIT_MAX_BLOCKS;
constexpr int kPart = SGMCMC_FIT_PART;                  // doubles of one workgroup's partial record
constexpr int kSlots = 2;                               // entries a thread owns: ceil(kPart / kThreads)
constexpr int kStage = 6;                               // elements a thread loads before it stores them to LDS
typedef sgmcmc_fit_geometry Geom;

// state record of a multivariate-t fit (SGMCMC_FIT_STATE doubles)
enum { kPhase = 0, kIter = 1, kConv = 2, kNu = 3, kLogDet = 4, kLogLik = 5, kAtBound = 6, kDelta = 7, kMu = 8,
       kLinv = kMu + kMaxP, kS = kLinv + kMaxP * kMaxP };
static_assert(kS + kMaxP * kMaxP <= SGMCMC_FIT_STATE, "state record");

__host__ __device__ inline int row_stride(int P) { return P | 1; }   // odd: a wave's rows fall on different LDS banks
__host__ __device__ inline int tile_events(int P, int F) {
  const int by_lds = kTileDoubles / (F * row_stride(P)), by_rows = kMaxRows / F;
  const int te = by_lds < by_rows ? by_lds : by_rows;
  return te < 1 ? 1 : te;
}
inline int blocks(int P, int F, int64_t events) {
  const int64_t tiles = (events + tile_events(P, F) - 1) / tile_events(P, F);
  return (int)(tiles < kMaxBlocks ? tiles : kMaxBlocks);
}

using num::comp_add;
using num::qnan;

// element offset of event e (< 2^31): its index is decomposed over the event dimensions, outermost first
__device__ __forceinline__ int64_t event_offset(const Geom& g, uint32_t e) {
  int64_t off = 0;
#pragma unroll
  for (int k = 3; k >= 0; --k) {
    const uint32_t s = (uint32_t)g.size[k];
    if (s != 1) {                                       // (uniform: unused dimensions cost no division)
      const uint32_t q = e / s;
      off += (int64_t)(e - q * s) * g.stride[k];
      e = q;
    }
  }
  return off;
}

// entry `ent` of a partial record -> what it sums: 0 w d_a d_b, 1 w d_a, 2 d_a^3, 3 d_a^4, 4 sum u, 5 sum (log u - u),
// 6 sum log(1 + M / nu)
__device__ __forceinline__ void decode(int ent, int P, bool em, int& type, int& a, int& b) {
  const int npairs = P * (P + 1) / 2;
  a = b = 0;
  if (ent < npairs) {
    while ((a + 1) * (a + 2) / 2 <= ent) ++a;
    b = ent - a * (a + 1) / 2;
    type = 0;
  } else if (ent < npairs + P) {
    a = ent - npairs;
    type = 1;
  } else if (em) {
    type = 4 + (ent - npairs - P);
  } else {
    type = 2 + (ent - npairs - P) / P;
    a = (ent - npairs - P) % P;
  }
}

template <typename T, bool kEM>
__global__ __launch_bounds__(kThreads) void pass_kernel(const T* __restrict__ w, const Geom g,
                                                        const double* __restrict__ par, double* __restrict__ part,
                                                        long long* __restrict__ ipart, double* __restrict__ shift_out) {
  __shared__ double sd[kTileDoubles];
  __shared__ double sq[kEM ? kMaxRows : 1], sw[kEM ? kMaxRows : 1], su[kEM ? kMaxRows : 1], sc2[kEM ? kMaxRows : 1];
  __shared__ double sLinv[kEM ? kMaxP * kMaxP : 1];
  __shared__ double smu[kMaxP];
  __shared__ long long spos[kMaxP];
  __shared__ long long sbad[kThreads];
  if (kEM && par[kPhase] == 2.0) return;               // a finished fit: later launches are no-ops
  const int t = threadIdx.x, P = g.P, F = g.F, Ps = row_stride(P);
  const int npairs = P * (P + 1) / 2, NE = kEM ? npairs + P + 3 : npairs + 3 * P;
  const int G = kThreads / NE < 1 ? 1 : kThreads / NE;  // row slices of an entry
  const int TE = tile_events(P, F);
  const uint32_t events = (uint32_t)g.events;
  const uint32_t tiles = (events + TE - 1) / TE;
  const double nu = kEM ? par[kNu] : 0.0, D = (double)F * (double)P;
#pragma unroll
  for (int a = 0; a < kMaxP; ++a)
    if (t == a) spos[a] = g.pos[a];
  __syncthreads();
  if (kEM) {
    if (t < P) smu[t] = par[kMu + t];
    for (int i = t; i < P * P; i += kThreads) sLinv[i] = par[kLinv + i];
  } else if (t < P) {
    // the shift: per position the median of vectors 0, n / 2 and n - 1 (the same in every workgroup)
    const uint32_t n = events * (uint32_t)F;
    double x[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const uint32_t v = j == 0 ? 0u : j == 1 ? n / 2 : n - 1;
      x[j] = (double)w[event_offset(g, v / F) + (int64_t)(v % F) * g.f_stride + spos[t]];
    }
    const double lo = fmin(x[0], x[1]), hi = fmax(x[0], x[1]);
    double m = fmax(lo, fmin(hi, x[2]));
    if (!(fabs(m) <= 1.79769313486231570815e308)) m = 0.0;      // (a NaN or Inf is counted below)
    smu[t] = m;
    if (blockIdx.x == 0) shift_out[t] = m;
  }
  int type[kSlots], ea[kSlots], eb[kSlots], grp[kSlots];
  double acc[kSlots], comp[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int id = t + kThreads * s;
    acc[s] = comp[s] = 0.0;
    grp[s] = id / NE;
    if (id < NE * G) decode(id - grp[s] * NE, P, kEM, type[s], ea[s], eb[s]);
    else type[s] = -1, ea[s] = eb[s] = 0;
  }
  long long bad = 0;
  __syncthreads();
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t e0 = tile * (uint32_t)TE;
    const int te = (int)min((uint32_t)TE, events - e0), rows = te * F, total = rows * P;
    // stage d = x - shift: k walks the tile in the order of the stack's memory
    for (int k0 = t; k0 < total; k0 += kStage * kThreads) {   // kStage loads in flight per thread
      T x[kStage];
      int at[kStage], pa[kStage];
#pragma unroll
      for (int j = 0; j < kStage; ++j) {
        const int k = k0 + j * kThreads;
        int el = 0, f = 0, a = 0;
        if (k < total) {
          if (g.f_major) {
            f = k / (te * P);
            const int rem = k - f * te * P;
            el = rem / P;
            a = rem - el * P;
          } else {
            el = k / (F * P);
            const int rem = k - el * F * P;
            f = rem / P;
            a = rem - f * P;
          }
          x[j] = w[event_offset(g, e0 + el) + (int64_t)f * g.f_stride + spos[a]];
        } else {
          x[j] = (T)0;
        }
        at[j] = k < total ? (el * F + f) * Ps + a : -1;
        pa[j] = a;
      }
#pragma unroll
      for (int j = 0; j < kStage; ++j)
        if (at[j] >= 0) {
          const double v = (double)x[j];
          bad += !(fabs(v) <= 1.79769313486231570815e308);
          sd[at[j]] = v - smu[pa[j]];
        }
    }
    __syncthreads();
    if (kEM) {
      for (int r = t; r < rows; r += kThreads) {        // q_r = |L^-1 d_r|^2
        const double* d = sd + r * Ps;
        double q = 0.0;
        for (int a = 0; a < P; ++a) {
          double z = 0.0;
          for (int b = 0; b <= a; ++b) z += sLinv[a * P + b] * d[b];
          q += z * z;
        }
        sq[r] = q;
      }
      __syncthreads();
      double u[kMaxRows / kThreads], c1[kMaxRows / kThreads], c2[kMaxRows / kThreads];
#pragma unroll
      for (int j = 0; j < kMaxRows / kThreads; ++j) {   // per event: M in ascending f, u and the two log terms
        const int e = t + kThreads * j;
        u[j] = c1[j] = c2[j] = 0.0;
        if (e < te) {
          double M = 0.0;
          for (int f = 0; f < F; ++f) M += sq[e * F + f];
          u[j] = (nu + D) / (nu + M);
          c1[j] = log(u[j]) - u[j];
          c2[j] = log1p(M / nu);
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kMaxRows / kThreads; ++j) {
        const int e = t + kThreads * j;
        if (e < te) { su[e] = u[j]; sq[e] = c1[j]; sc2[e] = c2[j]; }
      }
      __syncthreads();
      for (int r = t; r < rows; r += kThreads) sw[r] = su[r / F];
      __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      double ts = 0.0;
      const int a = ea[s], b = eb[s];
      if (type[s] == 0) {
        for (int r = grp[s]; r < rows; r += G) {
          const double v = sd[r * Ps + a] * sd[r * Ps + b];
          ts += kEM ? sw[r] * v : v;
        }
      } else if (type[s] == 1) {
        for (int r = grp[s]; r < rows; r += G) ts += kEM ? sw[r] * sd[r * Ps + a] : sd[r * Ps + a];
      } else if (type[s] == 2) {
        for (int r = grp[s]; r < rows; r += G) { const double v = sd[r * Ps + a]; ts += (v * v) * v; }
      } else if (type[s] == 3) {
        for (int r = grp[s]; r < rows; r += G) { const double v = sd[r * Ps + a], v2 = v * v; ts += v2 * v2; }
      } else if (type[s] >= 4) {
        const double* src = type[s] == 4 ? su : type[s] == 5 ? sq : sc2;
        for (int e = grp[s]; e < te; e += G) ts += src[e];
      }
      if (type[s] >= 0) comp_add(acc[s], comp[s], ts);
    }
    __syncthreads();
  }
  // the slices of an entry, in ascending order
#pragma unroll
  for (int s = 0; s < kSlots; ++s)
    if (type[s] >= 0) sd[t + kThreads * s] = acc[s] + comp[s];
  sbad[t] = bad;
  __syncthreads();
  for (int ent = t; ent < NE; ent += kThreads) {
    double v = 0.0;
    for (int q = 0; q < G; ++q) v += sd[q * NE + ent];
    part[(size_t)blockIdx.x * kPart + ent] = v;
  }
  if (t == 0) {
    long long c = 0;
    for (int q = 0; q < kThreads; ++q) c += sbad[q];
    ipart[blockIdx.x] = c;
  }
}

// tot[ent] = the workgroups' partials: slice q of G = max(1, 256 / NE) adds workgroups q, q + G, ... (compensated), the
// slices are added from 0 in ascending order; returns the sum of their integer counts
__device__ __forceinline__ long long add_partials(const double* __restrict__ part, const long long* __restrict__ ipart, int nblk, int NE,
                                  double* tot) {
  __shared__ long long count;
  __shared__ double red[2 * kThreads];
  const int G = kThreads / NE < 1 ? 1 : kThreads / NE;
  for (int id = threadIdx.x; id < NE * G; id += kThreads) {
    const int q = id / NE, ent = id - q * NE;
    double s = 0.0, c = 0.0;
#pragma unroll 8
    for (int b = q; b < nblk; b += G) comp_add(s, c, part[(size_t)b * kPart + ent]);
    red[id] = s + c;
  }
  __syncthreads();
  for (int ent = threadIdx.x; ent < NE; ent += kThreads) {
    double v = 0.0;
    for (int q = 0; q < G; ++q) v += red[q * NE + ent];
    tot[ent] = v;
  }
  if (threadIdx.x == 0) {
    long long c = 0;
    for (int b = 0; b < nblk; ++b) c += ipart[b];
    count = c;
  }
  __syncthreads();
  return count;
}

// out: mean [P], cov [P][P], skew [P], kurt [P], var [P] (population), pooled {mean, var, skew, kurt}; bad[0] = the
// non-finite elements
__global__ __launch_bounds__(kThreads) void moments_kernel(const double* __restrict__ part,
                                                           const long long* __restrict__ ipart, int nblk, int P,
                                                           double n, int ddof, const double* __restrict__ shift,
                                                           double* __restrict__ out, long long* __restrict__ bad) {
  __shared__ double tot[kPart], cm[4][kMaxP];
  const int t = threadIdx.x, npairs = P * (P + 1) / 2, NE = npairs + 3 * P;
  const long long nbad = add_partials(part, ipart, nblk, NE, tot);
  const int nout = P * P + 4 * P + 4;
  if (t == 0) bad[0] = nbad;
  if (nbad) {
    for (int i = t; i < nout; i += kThreads) out[i] = qnan();
    return;
  }
  double* mean = out, *cov = out + P, *skew = cov + P * P, *kurt = skew + P, *var = kurt + P, *pooled = var + P;
  if (t < P) {
    const double m = tot[npairs + t] / n;                      // mean of d
    const double s2 = tot[t * (t + 1) / 2 + t] / n, s3 = tot[npairs + P + t] / n, s4 = tot[npairs + 2 * P + t] / n;
    const double m2 = s2 - m * m;
    const double m3 = (s3 - 3.0 * m * s2) + 2.0 * (m * m) * m;
    const double m4 = ((s4 - 4.0 * m * s3) + 6.0 * (m * m) * s2) - 3.0 * (m * m) * (m * m);
    cm[0][t] = shift[t] + m;
    cm[1][t] = m2 > 0.0 ? m2 : 0.0;
    cm[2][t] = m3;
    cm[3][t] = m4;
    mean[t] = cm[0][t];
    var[t] = cm[1][t];
    skew[t] = m2 > 0.0 ? m3 / (m2 * sqrt(m2)) : qnan();        // a column of zero variance is reported, not divided by
    kurt[t] = m2 > 0.0 ? m4 / (m2 * m2) - 3.0 : qnan();
  }
  for (int i = t; i < P * P; i += kThreads) {
    const int a = i / P, b = i - a * P, hi = a > b ? a : b, lo = a > b ? b : a;
    const double c = tot[hi * (hi + 1) / 2 + lo] - tot[npairs + a] * (tot[npairs + b] / n);
    cov[i] = (a == b && !(c > 0.0) ? 0.0 : c) / (n - (double)ddof);
  }
  __syncthreads();
  if (t == 0) {
    double pm = 0.0, M2 = 0.0, M3 = 0.0, M4 = 0.0;
    for (int a = 0; a < P; ++a) pm += cm[0][a];
    pm /= (double)P;
    for (int a = 0; a < P; ++a) {
      const double dl = cm[0][a] - pm, d2 = dl * dl;
      M2 += cm[1][a] + d2;
      M3 += (cm[2][a] + 3.0 * dl * cm[1][a]) + d2 * dl;
      M4 += ((cm[3][a] + 4.0 * dl * cm[2][a]) + 6.0 * d2 * cm[1][a]) + d2 * d2;
    }
    M2 /= (double)P; M3 /= (double)P; M4 /= (double)P;
    pooled[0] = pm;
    pooled[1] = M2;
    pooled[2] = M2 > 0.0 ? M3 / (M2 * sqrt(M2)) : qnan();
    pooled[3] = M2 > 0.0 ? M4 / (M2 * M2) - 3.0 : qnan();
  }
}

// S [P][P] (LDS, row-major) -> its Cholesky factor L, Linv = L^-1; returns sum log L_aa, NaN if S is not positive definite
__device__ __forceinline__ double factor(const double* S, int P, double* L, double* Linv) {
  double ld = 0.0;
  for (int a = 0; a < P; ++a) {
    for (int b = 0; b <= a; ++b) {
      double s = S[a * P + b];
      for (int k = 0; k < b; ++k) s -= L[a * P + k] * L[b * P + k];
      if (a == b) {
        if (!(s > 0.0) || !(s <= 1.79769313486231570815e308)) return qnan();
        L[a * P + a] = sqrt(s);
        ld += log(L[a * P + a]);
      } else {
        L[a * P + b] = s / L[b * P + b];
      }
    }
    for (int b = a + 1; b < P; ++b) L[a * P + b] = 0.0;
  }
  for (int c = 0; c < P; ++c)                                   // column c of L^-1 by forward substitution
    for (int a = 0; a < P; ++a) {
      double s = a == c ? 1.0 : 0.0;
      for (int k = c; k < a; ++k) s -= L[a * P + k] * Linv[k * P + c];
      Linv[a * P + c] = a < c ? 0.0 : s / L[a * P + a];
    }
  return ld;
}

__device__ __forceinline__ void fail(double* par, int P) {
  for (int i = kNu; i < kS + P * P; ++i) par[i] = qnan();
  par[kConv] = 0.0;
  par[kAtBound] = 0.0;
  par[kPhase] = 2.0;
}

// theta_0: mu = mean, S = cov (nu - 2) / nu (the moments' covariance as the t's covariance), nu = df
__global__ __launch_bounds__(64) void mvt_init_kernel(int P, const double* __restrict__ mean,
                                                      const double* __restrict__ cov, double df,
                                                      double* __restrict__ par) {
  __shared__ double S[kMaxP * kMaxP], L[kMaxP * kMaxP], Li[kMaxP * kMaxP];
  if (threadIdx.x != 0) return;
  for (int i = 0; i < kNu; ++i) par[i] = 0.0;
  par[kNu] = df;
  for (int a = 0; a < P; ++a) par[kMu + a] = mean[a];
  for (int i = 0; i < P * P; ++i) S[i] = cov[i] * ((df - 2.0) / df);
  const double ld = factor(S, P, L, Li);
  if (ld != ld) { fail(par, P); return; }
  par[kLogDet] = ld;
  for (int i = 0; i < P * P; ++i) { par[kLinv + i] = Li[i]; par[kS + i] = S[i]; }
}

// the root in [lo, hi] of g(nu) = log(nu / 2) - psi(nu / 2) + c (decreasing): Newton from nu0, bisection when a step
// leaves the bracket
__device__ __forceinline__ double solve_nu(double c, double nu0, double lo, double hi) {
  auto g = [c](double nu) { return (log(0.5 * nu) - num::digamma(0.5 * nu)) + c; };
  if (!(g(lo) > 0.0)) return lo;
  if (!(g(hi) < 0.0)) return hi;
  double a = lo, b = hi, x = fmin(fmax(nu0, lo), hi);
  for (int it = 0; it < 200; ++it) {
    const double gx = g(x);
    if (gx > 0.0) a = x; else if (gx < 0.0) b = x; else return x;
    const double dg = 1.0 / x - 0.5 * num::trigamma(0.5 * x);
    double xn = x - gx / dg;
    if (!(xn > a && xn < b)) xn = 0.5 * (a + b);
    if (fabs(xn - x) <= 1e-15 * xn) return xn;
    x = xn;
  }
  return x;
}

__global__ __launch_bounds__(kThreads) void mvt_update_kernel(const double* __restrict__ part,
                                                              const long long* __restrict__ ipart, int nblk, int P, int F,
                                                              double events, double max_iter, double tol, double df_lo,
                                                              double df_hi, double* __restrict__ par,
                                                              double* __restrict__ trace) {
  __shared__ double tot[kPart], S[kMaxP * kMaxP], L[kMaxP * kMaxP], Li[kMaxP * kMaxP];
  if (par[kPhase] == 2.0) return;
  const int npairs = P * (P + 1) / 2, NE = npairs + P + 3;
  const long long nbad = add_partials(part, ipart, nblk, NE, tot);
  if (threadIdx.x != 0) return;
  const double nu = par[kNu], D = (double)F * (double)P;
  const double* A = tot + npairs;
  const double sum_u = tot[npairs + P], sum_c1 = tot[npairs + P + 1], sum_c2 = tot[npairs + P + 2];
  // the log-likelihood at the parameters the pass ran with
  const double ll = events * (((num::log_gamma(0.5 * (nu + D)) - num::log_gamma(0.5 * nu)) - 0.5 * D * log(3.14159265358979323846 * nu))
                              - (double)F * par[kLogDet]) - 0.5 * (nu + D) * sum_c2;
  if (nbad || !(fabs(ll) <= 1.79769313486231570815e308)) {
    fail(par, P);
    par[kLogLik] = qnan();
    return;
  }
  if (par[kPhase] == 1.0) {                                      // the pass at the returned parameters
    par[kLogLik] = ll;
    par[kPhase] = 2.0;
    return;
  }
  const int it = (int)par[kIter];
  trace[it] = ll;
  const double W = (double)F * sum_u;
  for (int a = 0; a < P; ++a)
    for (int b = 0; b <= a; ++b) {
      const double v = (tot[a * (a + 1) / 2 + b] - A[a] * (A[b] / W)) / W;
      S[a * P + b] = v;
      S[b * P + a] = v;
    }
  const double ld = factor(S, P, L, Li);
  if (ld != ld) { fail(par, P); par[kLogLik] = qnan(); return; }
  const double h = 0.5 * (nu + D);
  const double c = ((1.0 + sum_c1 / events) + num::digamma(h)) - log(h);
  const double nu_new = solve_nu(c, nu, df_lo, df_hi);
  // the relative change of (mu, S, nu)
  double delta = fabs(nu_new - nu) / nu_new;
  for (int a = 0; a < P; ++a) {
    const double step = A[a] / W;
    delta = fmax(delta, fabs(step) / sqrt(S[a * P + a]));
    par[kMu + a] += step;
    for (int b = 0; b <= a; ++b)
      delta = fmax(delta, fabs(S[a * P + b] - par[kS + a * P + b]) / sqrt(S[a * P + a] * S[b * P + b]));
  }
  for (int i = 0; i < P * P; ++i) { par[kS + i] = S[i]; par[kLinv + i] = Li[i]; }
  par[kNu] = nu_new;
  par[kLogDet] = ld;
  par[kDelta] = delta;
  par[kAtBound] = nu_new == df_lo || nu_new == df_hi ? 1.0 : 0.0;
  par[kIter] = (double)(it + 1);
  if (delta <= tol) { par[kConv] = 1.0; par[kPhase] = 1.0; }
  else if ((double)(it + 1) >= max_iter) par[kPhase] = 1.0;
}

// element v of a P = F = 1 geometry: d = |x - loc|; part: sum d, sum log d, sum d^beta, sum d^beta log d,
// sum d^beta log^2 d over the d > 0; ipart: the d == 0.  Thread t of workgroup b takes elements b 256 + t, + grid 256, ..
template <typename T>
__global__ __launch_bounds__(kThreads) void abs_kernel(const T* __restrict__ w, const Geom g, double loc, double beta,
                                                       double* __restrict__ part, long long* __restrict__ ipart) {
  __shared__ double red[5][kThreads];
  __shared__ long long sz[kThreads];
  const int t = threadIdx.x;
  const uint32_t n = (uint32_t)g.events;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  long long zeros = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * kThreads + t; v < n; v += (uint64_t)gridDim.x * kThreads) {
    const double d = fabs((double)w[event_offset(g, (uint32_t)v)] - loc);
    if (d == 0.0) { ++zeros; continue; }
    const double l = log(d), p = exp(beta * l);
    comp_add(s[0], c[0], d);
    comp_add(s[1], c[1], l);
    comp_add(s[2], c[2], p);
    comp_add(s[3], c[3], p * l);
    comp_add(s[4], c[4], (p * l) * l);
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) red[j][t] = s[j] + c[j];
  sz[t] = zeros;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int j = 0; j < 5; ++j) red[j][t] += red[j][t + off];
      sz[t] += sz[t + off];
    }
    __syncthreads();
  }
  if (t < 5) part[(size_t)blockIdx.x * kPart + t] = red[t][0];
  if (t == 0) ipart[blockIdx.x] = sz[0];
}

__global__ __launch_bounds__(kThreads) void abs_total_kernel(const double* __restrict__ part,
                                                             const long long* __restrict__ ipart, int nblk,
                                                             double* __restrict__ out, long long* __restrict__ zeros) {
  __shared__ double tot[kPart];
  const long long z = add_partials(part, ipart, nblk, 5, tot);
  if (threadIdx.x < 5) out[threadIdx.x] = tot[threadIdx.x];
  if (threadIdx.x == 0) zeros[0] = z;
}

inline bool geometry_ok(const Geom* g) {
  if (!g || g->P < 1 || g->P > kMaxP || g->F < 1 || g->F > kMaxRows || g->F * row_stride(g->P) > kTileDoubles ||
      g->events < 1 || g->events * g->F >= (int64_t)1 << 31 || g->f_stride < 0)
    return false;
  int64_t prod = 1;
  for (int k = 0; k < 4; ++k) {
    if (g->size[k] < 1 || g->stride[k] < 0) return false;
    prod *= g->size[k];
  }
  for (int a = 0; a < g->P; ++a)
    if (g->pos[a] < 0) return false;
  return prod == g->events;
}

}  // namespace fit

extern "C" int sgmcmc_fit_blocks(int P, int F, int64_t events) {
  if (P < 1 || P > fit::kMaxP || F < 1 || F > fit::kMaxRows || F * fit::row_stride(P) > fit::kTileDoubles || events < 1)
    return -1;
  return fit::blocks(P, F, events);
}

extern "C" int sgmcmc_fit_moments(const void* w, int dtype, const sgmcmc_fit_geometry* geometry, int ddof, double* part,
                                  int64_t* counts, double* out, int64_t* bad, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!w || !fit::geometry_ok(geometry) || !part || !counts || !out || !bad || ddof < 0 ||
      (dtype != SGMCMC_F32 && dtype != SGMCMC_F64))
    return (int)hipErrorInvalidValue;
  const fit::Geom g = *geometry;
  const int nblk = fit::blocks(g.P, g.F, g.events);
  double* shift = part + (size_t)nblk * fit::kPart;     // (the workspace holds one record more than workgroups)
  if (dtype == SGMCMC_F32)
    SGMCMC_LAUNCH((fit::pass_kernel<float, false>), dim3(nblk), dim3(fit::kThreads), 0, (hipStream_t)stream,
                  (const float*)w, g, (const double*)nullptr, part, (long long*)counts, shift);
  else
    SGMCMC_LAUNCH((fit::pass_kernel<double, false>), dim3(nblk), dim3(fit::kThreads), 0, (hipStream_t)stream,
                  (const double*)w, g, (const double*)nullptr, part, (long long*)counts, shift);
  SGMCMC_LAUNCH(fit::moments_kernel, dim3(1), dim3(fit::kThreads), 0, (hipStream_t)stream, (const double*)part,
                (const long long*)counts, nblk, g.P, (double)(g.events * g.F), ddof, (const double*)shift, out,
                (long long*)bad);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_fit_mvt_init(int P, const double* mean, const double* cov, double df, double* state,
                                   void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (P < 1 || P > fit::kMaxP || !mean || !cov || !state || !(df > 2.0))
    return (int)hipErrorInvalidValue;
  SGMCMC_LAUNCH(fit::mvt_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, P, mean, cov, df, state);
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_fit_mvt_iterate(const void* w, int dtype, const sgmcmc_fit_geometry* geometry, int iters,
                                      int64_t max_iter, double tol, double df_lo, double df_hi, double* part,
                                      int64_t* counts, double* state, double* trace, void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!w || !fit::geometry_ok(geometry) || !part || !counts || !state || !trace || iters < 0 || max_iter < 1 ||
      max_iter > ((int64_t)1 << 30) || !(tol >= 0.0) || !(df_lo > 2.0) || !(df_hi >= df_lo) ||
      (dtype != SGMCMC_F32 && dtype != SGMCMC_F64))
    return (int)hipErrorInvalidValue;
  const fit::Geom g = *geometry;
  const int nblk = fit::blocks(g.P, g.F, g.events);
  for (int i = 0; i < iters; ++i) {
    if (dtype == SGMCMC_F32)
      SGMCMC_LAUNCH((fit::pass_kernel<float, true>), dim3(nblk), dim3(fit::kThreads), 0, (hipStream_t)stream,
                    (const float*)w, g, (const double*)state, part, (long long*)counts, (double*)nullptr);
    else
      SGMCMC_LAUNCH((fit::pass_kernel<double, true>), dim3(nblk), dim3(fit::kThreads), 0, (hipStream_t)stream,
                    (const double*)w, g, (const double*)state, part, (long long*)counts, (double*)nullptr);
    SGMCMC_LAUNCH(fit::mvt_update_kernel, dim3(1), dim3(fit::kThreads), 0, (hipStream_t)stream, (const double*)part,
                  (const long long*)counts, nblk, g.P, g.F, (double)g.events, (double)max_iter, tol, df_lo, df_hi, state,
                  trace);
  }
  return (int)hipGetLastError();
}

extern "C" int sgmcmc_fit_abs_stats(const void* w, int dtype, const sgmcmc_fit_geometry* geometry, double loc,
                                    double beta, double* part, int64_t* counts, double* out, int64_t* zeros,
                                    void* stream) {
  SGMCMC_FRESH_ERROR_STATE();
  if (!w || !fit::geometry_ok(geometry) || geometry->P != 1 || geometry->F != 1 || !part || !counts || !out || !zeros ||
      !(beta > 0.0) || (dtype != SGMCMC_F32 && dtype != SGMCMC_F64))
    return (int)hipErrorInvalidValue;
  const fit::Geom g = *geometry;
  const int nblk = fit::blocks(1, 1, g.events);
  if (dtype == SGMCMC_F32)
    SGMCMC_LAUNCH((fit::abs_kernel<float>), dim3(nblk), dim3(fit::kThreads), 0, (hipStream_t)stream, (const float*)w, g,
                  loc, beta, part, (long long*)counts);
  else
    SGMCMC_LAUNCH((fit::abs_kernel<double>), dim3(nblk), dim3(fit::kThreads), 0, (hipStream_t)stream, (const double*)w, g,
                  loc, beta, part, (long long*)counts);
  SGMCMC_LAUNCH(fit::abs_total_kernel, dim3(1), dim3(fit::kThreads), 0, (hipStream_t)stream, (const double*)part,
                (const long long*)counts, nblk, out, (long long*)zeros);
  return (int)hipGetLastError();
}
