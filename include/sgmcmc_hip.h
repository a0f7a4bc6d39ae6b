/*
 * sgmcmc_hip.h -- C ABI of the MI355X (gfx950) SG-MCMC leapfrog engine.
 *
 * This is the drop-in boundary underneath the Python optimizer classes
 * bnn_priors_amd.mcmc.{SGLD,VerletSGLD,HMC}: plain pointers, sizes and PODs,
 * no torch types.  Every entry point
 *   - takes device pointers that the caller owns (nothing is allocated here),
 *   - enqueues its kernels on the given hipStream_t (passed as void*) and
 *     returns immediately (no host synchronisation inside),
 *   - returns a hipError_t as int (0 = success).
 *
 * The reference has no FFI: its samplers are pure-Python torch.optim.Optimizer
 * subclasses.  Each entry point therefore cites the reference *method* whose
 * per-tensor Python loop it replaces (paths under /root/reference/bnn_priors/).
 *
 * Data model
 * ----------
 * A sampler instance owns an ARENA tiled into CHUNKs of SGMCMC_CHUNK elements.
 * Parameter tensor ("segment") s occupies ceil(numel_s / chunk_elems)
 * consecutive chunks starting at first_chunk_s (chunk_elems is a property of the layout:
 * 4096, or 1024 for small models so that they still fill many CUs); the optimizer-owned state
 * arrays m (momentum), v (RMSprop square_avg), prev_theta / prev_g / prev_m
 * (Metropolis-Hastings roll-back copies) live in the arena at element offset
 * chunk * chunk_elems.  theta (the nn.Parameter storage) and g (its .grad)
 * are NOT moved: kernels reach them through the per-segment base pointers, so
 * autograd can keep allocating gradients wherever it likes.
 */
#ifndef SGMCMC_HIP_H
#define SGMCMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGMCMC_ABI_VERSION 28
#define SGMCMC_CHUNK 4096 /* default elements per arena chunk = 256 threads x 4 items x 4 elements */
#define SGMCMC_CHUNK_SMALL 1024 /* small models: one item per thread, 4x more workgroups */
#define SGMCMC_NSUMS 6
#define SGMCMC_PSTRIDE 8   /* doubles per chunk in `partials`: the 6 sums, [6] log-prior, [7] spare */
#define SGMCMC_MLP_ROWS 16 /* batch rows per workgroup of the fused dense-net kernel */

enum { SGMCMC_F32 = 0, SGMCMC_F64 = 1 };
enum { SGMCMC_VERLET = 0, SGMCMC_HMC = 1, SGMCMC_SGLD = 2 };
/* flags of sgmcmc_step_args */
enum {
  SGMCMC_INITIAL = 1,      /* first transition after an M-H point (verlet_sgld.py:86, hmc.py:46) */
  SGMCMC_FINAL = 2,        /* last transition: theta and v are not modified (verlet_sgld.py:119) */
  SGMCMC_SAVE_STATE = 4,   /* copy theta,g,m to prev_* first (verlet_sgld.py:72-83) */
  SGMCMC_CALC_METRICS = 8, /* update est_temperature / est_config_temp */
  SGMCMC_UNALIGNED = 16,   /* some theta/g base pointer is not 16-byte aligned: scalar loads */
  SGMCMC_NO_MOMENTUM = 32, /* SGLD with momentum == 0: m is neither read nor written */
  SGMCMC_SMALL_FINALIZE = 64, /* few chunks: one workgroup finalizes all segments and leaves
                                 scalars[3] = sum_s(delta_energy_s + point_energy_s) for the
                                 gradient / momentum of THIS transition */
  SGMCMC_DEFER_FINALIZE = 256, /* launch only the update kernel; the per-segment bookkeeping is run
                                  later by sgmcmc_finalize or inside the next sgmcmc_dense_step_direct
                                  (it is not an input of the next gradient evaluation) */
  SGMCMC_WITH_LOG_PRIOR = 128, /* with SMALL_FINALIZE + CALC_METRICS: partials[.][6] holds the
                                 fused priors' log-density partials (sgmcmc_grad_reduce_prior):
                                 finish state[s].aux and scalars[2] in the same launch */
  SGMCMC_INLINE_PRIOR = 512 /* sgmcmc_step_indirect only (float32 arena; priors of kind <= CAUCHY without linked
                               scales): g holds the likelihood gradient alone and the update kernel adds the
                               closed-form prior gradient in flight (and, on a CALC_METRICS step, leaves the
                               log-density partials for WITH_LOG_PRIOR) -- no sgmcmc_prior_grad launch before it.
                               g holds the full gradient afterwards, as after sgmcmc_prior_grad. */
};
/* element-wise priors the kernels differentiate in closed form (prior/loc_scale.py, prior/distributions.py:75-79)
 * and the element-wise hyper-priors of a hierarchical scale (prior/transformed.py:55-87, hierarchical.py:17-104):
 *   GENNORM            log p = -log(2 scale) - lgamma(1/beta) + log beta - (|theta - loc| / scale)^beta; beta in prior_df
 *   GAMMA_SOFTPLUS     theta is the raw parameter s, the value x = softplus(s) ~ Gamma(concentration = prior_loc,
 *                      rate = prior_scale): log p = c log r - lgamma(c) + (c-1) log x - r x
 *   UNIFORM_CDF        value x = low + (high - low) Phi(s), low = prior_loc, high = prior_scale: log p = -log(high-low)
 *   HALFCAUCHY_SOFTPLUS value x = softplus(s) * multiplier (prior_loc) ~ HalfCauchy(scale = prior_scale), the density
 *                      evaluated AT x: log p = log(2 / (pi g)) - log(1 + (x/g)^2)
 *   IMPROPER_SOFTPLUS  value x = softplus(s), NO density (log p = 0, no gradient of its own): the learnable scale of the
 *                      empirical-Bayes priors (prior/loc_scale.py:100-103 under prior/empirical_bayes.py:24-38)
 * A weight segment whose scale_link > 0 takes its scale from the VALUE of hyper segment scale_link - 1 (one element)
 * at launch time instead of prior_scale; sgmcmc_prior_grad then also adds
 * -(1/N) (d/dscale sum_j log p(theta_j)) dx/ds to the hyper segment's gradient (flags & SGMCMC_PRIOR_HAS_LINKS).
 *
 * FILTER_WHITENED and MULTIVARIATE_T are not element-wise.  A segment of either kind (a convolution weight
 * [Cout, Cin, kh, kw] in contiguous order, say) is a sequence of filters of P consecutive elements, each whitened by the
 * segment's record L->filters[s]: z = (theta_f - mu) W (row vector), and element j at position q = j mod P receives
 *   g_j += -(1/N) coef sum_k psi(z_k) W[q][k],
 * everything in fp64 with one rounding into g.  Element j reads the other positions of its filter from theta, so both
 * kinds are evaluated by sgmcmc_prior_grad's full kernel only (a launch that does not write theta); prior_loc /
 * prior_scale / prior_df are unused.  What each kind adds:
 *
 * FILTER_WHITENED (prior/correlated.py): coef = 1, psi = d base / dz, log p(theta_f) = sum_k base(z_k) + lognorm,
 * with the base density chosen by the record's base (SGMCMC_FILTER_BASE_*; their constants are in lognorm):
 *   NORMAL        base(z) = -z^2 / 2                              (beta, base_scale unused)
 *   GENNORM       base(z) = -|z / base_scale|^beta                (beta = shape, base_scale = scale)
 *   LAPLACE       base(z) = -|z| / base_scale                     (base_scale = b; beta unused)
 *   DOUBLE_GAMMA  base(z) = (beta - 1) log|z| - |z| / base_scale  (beta = concentration c, base_scale = 1 / rate)
 * psi is 0 at z == 0 for every base (where autograd of GENNORM / DOUBLE_GAMMA gives NaN); the DOUBLE_GAMMA log term there
 * follows torch's xlogy: 0 when c == 1, +-inf otherwise.  Any other base value yields NaN (never a silent Normal).
 *
 * MULTIVARIATE_T (prior/multivariate_t.py; Shah et al.'s parameterisation, lambda = df - 2): psi = z, and the record
 * also holds an EVENT geometry: element j belongs to event (j / ev_div) % ev_mod, and one event of D = ev_size elements
 * is a whole number of filters.  With M_e = sum over the event's filters of |z|^2,
 *   log p(event) = lognorm - ((df + D) / 2) log(1 + M_e / lambda),   coef = -(df + D) / (lambda + M_e),
 * lognorm = lgamma((D + df)/2) - lgamma(df/2) - (D/2) log(pi lambda) - half log |det| of the event.  sgmcmc_prior_grad
 * first writes every event's M_e to the record's ev_sum (one launch, fp64, a fixed summation order: bit-reproducible),
 * then the full kernel applies the gradient; the event's first element (j % ev_div == 0, j < ev_div ev_mod) carries
 * its whole log-density.  Such a table sets SGMCMC_PRIOR_EVENTS in prior_flags (and, beyond CAUCHY, PRIOR_FULL). */
enum { SGMCMC_PRIOR_NONE = 0, SGMCMC_PRIOR_NORMAL = 1, SGMCMC_PRIOR_LAPLACE = 2,
       SGMCMC_PRIOR_STUDENT_T = 3, SGMCMC_PRIOR_CAUCHY = 4, SGMCMC_PRIOR_GENNORM = 5,
       SGMCMC_PRIOR_GAMMA_SOFTPLUS = 6, SGMCMC_PRIOR_UNIFORM_CDF = 7, SGMCMC_PRIOR_HALFCAUCHY_SOFTPLUS = 8,
       SGMCMC_PRIOR_IMPROPER_SOFTPLUS = 9, SGMCMC_PRIOR_FILTER_WHITENED = 10, SGMCMC_PRIOR_MULTIVARIATE_T = 11 };
/* flags of sgmcmc_prior_grad: some segment is linked to a hyper segment / some segment's kind is beyond CAUCHY
 * (without either the lean kernel for the four constant-scale families is launched) / some segment is
 * MULTIVARIATE_T (its per-event sums are computed first) */
enum { SGMCMC_PRIOR_HAS_LINKS = 1, SGMCMC_PRIOR_FULL = 2, SGMCMC_PRIOR_EVENTS = 4 };

/* One parameter tensor.  Device-resident array, written by the host. */
typedef struct {
  void* theta;          /* base of the parameter storage (dtype of the layout) */
  void* g;              /* base of its gradient */
  double M;             /* state['preconditioner'] (sgld.py:47-52) */
  int64_t numel;
  int64_t first_chunk;
  int64_t noise_base;   /* Philox element index of element 0 (multiple of 4) */
  int32_t prior_kind;   /* SGMCMC_PRIOR_*; NONE = g already holds the full gradient */
  int32_t scale_link;   /* > 0: the prior's scale is the value of hyper segment scale_link - 1 (see above) */
  double prior_loc, prior_scale, prior_df;
} sgmcmc_segment;

#define SGMCMC_FILTER_MAX_P 25 /* positions per filter of SGMCMC_PRIOR_FILTER_WHITENED (5 x 5) */
enum { SGMCMC_FILTER_BASE_NORMAL = 0, SGMCMC_FILTER_BASE_GENNORM = 1, SGMCMC_FILTER_BASE_LAPLACE = 2,
       SGMCMC_FILTER_BASE_DOUBLE_GAMMA = 3 };
/* The whitening of one FILTER_WHITENED or MULTIVARIATE_T segment (device array L->filters, one record per segment, read
 * only for segments of those kinds).  The host computes it in float64 and rewrites it in place when the covariance
 * changes. */
typedef struct {
  int32_t P;          /* positions per filter, 1..SGMCMC_FILTER_MAX_P; the segment's numel is a multiple of it */
  int32_t base;       /* SGMCMC_FILTER_BASE_* */
  double beta, base_scale; /* the base's shape and scale (see FILTER_WHITENED above; NORMAL uses neither) */
  double lognorm;     /* log-normaliser of one filter's density */
  double mu[SGMCMC_FILTER_MAX_P];                       /* location of each position */
  double W[SGMCMC_FILTER_MAX_P * SGMCMC_FILTER_MAX_P];  /* whitening matrix, row-major with row stride P */
  /* MULTIVARIATE_T only (lognorm is then the log-normaliser of one EVENT) */
  double df;          /* degrees of freedom, > 2 */
  int64_t ev_size;    /* D: elements per event, a multiple of P */
  int64_t ev_div, ev_mod; /* element j belongs to event (j / ev_div) % ev_mod; ev_div is a multiple of P and
                             ev_div * ev_mod divides the segment's numel */
  double* ev_sum;     /* device [ev_mod]: each event's Mahalanobis norm M_e, scratch written by sgmcmc_prior_grad */
} sgmcmc_filter_prior;

typedef struct {
  int32_t seg;     /* owning segment */
  int32_t n_valid; /* elements of this chunk inside the segment (1..SGMCMC_CHUNK) */
} sgmcmc_chunk;

/* Per-segment running scalars, device-resident, fp64.  The host reads this
 * array back only when a caller asks for a metric or an energy. */
typedef struct {
  double sums[SGMCMC_NSUMS]; /* g.g, g.m_old, g.m_new, m_old.m_old, m_new.m_new, theta_old.g */
  double delta_energy;       /* state['delta_energy']            (verlet_sgld.py:170-175) */
  double prev_delta;         /* state['prev_new_momentum_delta'] (verlet_sgld.py:176) */
  double est_temperature;    /* (verlet_sgld.py:178-187) */
  double est_config_temp;    /* (verlet_sgld.py:189) */
  double point_energy;       /* last value computed by sgmcmc_delta_energy */
  double aux;                /* sgmcmc_segment_sum result (e.g. sum of v) */
} sgmcmc_seg_state;

typedef struct {
  int32_t dtype; /* SGMCMC_F32 | SGMCMC_F64 */
  int32_t n_seg;
  int64_t n_chunks;
  int64_t chunk_elems; /* SGMCMC_CHUNK or SGMCMC_CHUNK_SMALL: elements per chunk of THIS layout */
  const sgmcmc_segment* segs; /* device [n_seg] */
  const sgmcmc_chunk* chunks; /* device [n_chunks] */
  void* m;                    /* device arenas, n_chunks * SGMCMC_CHUNK elements each */
  void* v;
  void* prev_theta;
  void* prev_g;
  void* prev_m;
  double* partials;        /* device [n_chunks][SGMCMC_PSTRIDE] scratch */
  sgmcmc_seg_state* state; /* device [n_seg] */
  double* scalars;         /* device [8] outputs: [0] sgmcmc_delta_energy total, [1] non-finite flag,
                              [2] fused log-prior total, [3] energy total of the last transition
                              (SGMCMC_SMALL_FINALIZE only), [4] minibatch loss, [5] minibatch
                              accuracy (sgmcmc_grad_reduce_prior) */
  uint32_t prior_flags;    /* SGMCMC_PRIOR_HAS_LINKS | _FULL | _EVENTS as they hold for THIS segment table: the
                              entry points that only carry the lean prior code (sgmcmc_grad_reduce_prior, the
                              gradient-assembling step kernels, SGMCMC_INLINE_PRIOR) return hipErrorInvalidValue
                              when either bit is set instead of evaluating a family they do not implement */
  uint32_t reserved;
  const sgmcmc_filter_prior* filters; /* device [n_seg] (or NULL when no segment is FILTER_WHITENED / MULTIVARIATE_T) */
} sgmcmc_layout;

/* Scalars of one transition of one parameter group, computed by the host in
 * double exactly as the reference's _update_group_fn does. */
typedef struct {
  int32_t kind;  /* SGMCMC_VERLET | SGMCMC_HMC | SGMCMC_SGLD */
  uint32_t flags;
  int32_t seg_begin, seg_end;     /* the group's segments [begin, end) */
  int64_t chunk_begin, chunk_end; /* and their chunks */
  double num_data;   /* N */
  double b2h2;       /* lr / N           (verlet_sgld.py:139) */
  double bh;         /* sqrt(lr / N)     (verlet_sgld.py:140; sgld.py:116 'h') */
  double bhn;        /* sqrt(lr * N)     (verlet_sgld.py:141; sgld.py:115 'hn') */
  double mom_decay;  /* verlet_sgld.py:144,98,131 ; SGLD: momentum a */
  double grad_v;     /* verlet_sgld.py:145,99,132 */
  double noise_std;  /* verlet_sgld.py:146,100,133 ; sgld.py:117 ; 0 => no draw */
  double rmsprop_alpha;
  double grad_clamp; /* > 0: clamp g to +-grad_clamp in flight (inference.py:219-220); 0 = off */
  uint64_t seed;     /* Philox key */
  uint64_t draw;     /* sweep counter */
  uint32_t stream;   /* chain id */
  uint32_t reserved;
} sgmcmc_step_args;

int sgmcmc_abi_version(void);
/* hash of the sources the library was built from (csrc/ + include/), as the build handed it in; "unstamped" if it did not */
const char* sgmcmc_source_sha(void);
const char* sgmcmc_error_string(int err);

/* One transition of one parameter group: fused noise + momentum + position +
 * RMSprop update and the six per-segment dot products, then the per-segment
 * energy / temperature bookkeeping.
 * Replaces SGLD._step_internal + _step_fn (mcmc/sgld.py:88-154),
 * VerletSGLD.initial_step/step/final_step + _step_fn (mcmc/verlet_sgld.py:85-197),
 * HMC._step_fn (mcmc/hmc.py:41-79). */
int sgmcmc_step(const sgmcmc_layout* L, const sgmcmc_step_args* A, void* stream);

/* As sgmcmc_step, with the fused update kernel (not the finalize kernel) launched so that ev_start /
 * ev_stop carry ITS begin / end timestamps (hipExtLaunchKernelGGL): hipEventElapsedTime(ev_start,
 * ev_stop) is that kernel's execution time, measured live (bench.py roofline).  Events are hipEvent_t
 * created by sgmcmc_event_create. */
int sgmcmc_step_timed(const sgmcmc_layout* L, const sgmcmc_step_args* A, void* stream,
                      void* ev_start, void* ev_stop);
/* As sgmcmc_step, but the kernels read the transition's scalars from DEVICE memory
 * (*A_dev, same struct) when they run.  Launch geometry and kernel selection (kind, dtype,
 * seg/chunk ranges, SGMCMC_UNALIGNED, SGMCMC_NO_MOMENTUM) are taken from *A_host and must not
 * differ in *A_dev (the kernels take chunk_begin from *A_host and request their chunk's m and v before *A_dev has
 * arrived: L->m and L->v must be non-NULL and padded to whole chunks whatever the flags; NULL: hipErrorInvalidValue).
 * This is what makes the launch capturable in a hipGraph that is replayed with a different learning rate / draw
 * counter / flags every step. */
int sgmcmc_step_indirect(const sgmcmc_layout* L, const sgmcmc_step_args* A_host,
                         const sgmcmc_step_args* A_dev, void* stream);

/* Likelihood gradient given as per-slice partials (written by sgmcmc_mlp_fwdbwd): element j of
 * segment s lives at gpart[slice*stride + noise_base_s + j]. */
typedef struct {
  const float* gpart;
  const float* loss_part;    /* [n_slices] */
  const float* correct_part; /* [n_slices] */
  int64_t stride;
  double num_data;
  int32_t n_slices, batch;
} sgmcmc_grad_parts;

/* sgmcmc_step_indirect with the gradient assembled in flight: g <- sum over slices (fixed
 * order) - (1/N) dlog p/dtheta, used by the transition AND written back to each segment's g;
 * on metric steps also the log-prior partials; scalars[4], [5] <- minibatch loss / accuracy.
 * fp32 layouts only.  One launch instead of sgmcmc_grad_reduce_prior + sgmcmc_step_indirect. */
int sgmcmc_step_indirect_parts(const sgmcmc_layout* L, const sgmcmc_step_args* A_host,
                               const sgmcmc_step_args* A_dev, const sgmcmc_grad_parts* G,
                               void* stream);
int sgmcmc_event_create(void** ev);
int sgmcmc_event_destroy(void* ev);
/* hipEventRecord on `stream`: lets a caller bracket ANY entry point of this library with events on the
 * stream its kernels are launched on (bench.py's live roofline timing of the convolution kernels). */
int sgmcmc_event_record(void* ev, void* stream);
/* The NEXT kernel this library launches (from the calling thread's next entry-point call) carries the two
 * events in its dispatch packet, as sgmcmc_step_timed does for the update kernel: the elapsed time between
 * them is that kernel's own duration.  Used by bench.py to time the convolution kernels live. */
int sgmcmc_time_next_launch(void* ev_start, void* ev_stop);
int sgmcmc_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms); /* synchronises on ev_stop */

/* m <- sqrt(keep)*m + std*xi   (keep == 0: m <- std*xi).
 * Replaces SGLD.sample_momentum (mcmc/sgld.py:57-69). */
int sgmcmc_sample_momentum(const sgmcmc_layout* L, double std, double keep, uint64_t seed,
                           uint32_t stream, uint64_t draw, void* stream_);

/* theta,g,m <- prev_theta,prev_g,prev_m.
 * Replaces the roll-back loop of VerletSGLD.maybe_reject (mcmc/verlet_sgld.py:62-69). */
int sgmcmc_restore(const sgmcmc_layout* L, int restore_momentum, uint32_t flags, void* stream);

/* scalars[0] <- sum_s (state[s].delta_energy + point_energy_s), in segment order,
 * point_energy_s = (M^2 N^2 b2h2 / 8) g.g (Verlet) or 0.5 m.m (HMC), from the
 * CURRENT g / m.  Replaces VerletSGLD.delta_energy's loop + _point_energy
 * (mcmc/verlet_sgld.py:27-47, mcmc/hmc.py:32-33); the caller adds (U - U_prev) * N. */
int sgmcmc_delta_energy(const sgmcmc_layout* L, int kind, double num_data, double b2h2,
                        double grad_clamp, uint32_t flags, void* stream);

/* state[s].aux <- sum of v over segment s (which = 0), of m*m (1) or g*g (2).
 * which = 0 replaces the square_avg.mean() loop of SGLD.update_preconditioner
 * (mcmc/sgld.py:156-179); the host finishes (mean + eps, min, ^(-1/4)). */
int sgmcmc_segment_sum(const sgmcmc_layout* L, int which, uint32_t flags, void* stream);

/* g <- g - (1/N) dlog p(theta)/dtheta for every segment with prior_kind != NONE
 * (element-wise Normal / Laplace / Student-t / Cauchy / generalised normal with scalar loc, scale, df / beta,
 * the hyper-priors of hierarchical scales, the whitened convolution filters and the multivariate Student-t;
 * see SGMCMC_PRIOR_*), i.e. what
 * autograd adds for the "- log_prior / N" term of potential_avg (models/base.py:72-77,
 * prior/base.py:57-58, prior/loc_scale.py:34-35,66-67,74-77).  With calc_log_prob != 0 also
 * state[s].aux <- sum_j log p(theta_j) (fp64) and scalars[2] <- the total over segments.
 * One launch for all tensors instead of ~10 ATen launches per prior tensor per step. */
int sgmcmc_prior_grad(const sgmcmc_layout* L, double num_data, int calc_log_prob, uint32_t flags,
                      void* stream);

/* ---- fused dense classifier (ClassificationDenseNet, models/dense_nets.py:48-67) ---------- */
/* Forward + backward of -(1/B) sum_i log softmax(net(x_i) / T)[y_i] for
 * net = Linear(in,h1)-ReLU-Linear(h1,h2)-ReLU-Linear(h2,out), fp32, in ONE launch
 * (csrc/mlp_hip.inc).  Rows are gathered as X[idx[b]], Y[idx[b]] (idx == NULL: b itself).
 * Workgroup s writes its 16 rows' PARTIAL gradients to gpart + s*gpart_stride at the given
 * per-tensor offsets, and loss_part[s] = sum of its rows' losses, correct_part[s] = #correct.
 * Limits: in % 4 == 0, h1,h2 <= 64, out <= 16, LDS(in) <= 160 KiB. */
typedef struct {
  const float* X;      /* [n_data, in]  device */
  const int64_t* Y;    /* [n_data]      device */
  const int64_t* idx;  /* [batch] device, or NULL */
  const float *W1, *b1, *W2, *b2, *W3, *b3;
  float* gpart;        /* [ceil(batch/16)][gpart_stride] */
  float* loss_part;    /* [ceil(batch/16)] */
  float* correct_part; /* [ceil(batch/16)] */
  int64_t gpart_stride;
  int64_t off_W1, off_b1, off_W2, off_b2, off_W3, off_b3;
  int32_t batch, in_features, hidden1, hidden2, out_features;
  float inv_softmax_temp;
  int64_t* trace; /* optional (else NULL): 9 clock64() stamps at the phase boundaries of workgroup 0 */
  /* optional (else NULL): workgroup 0 copies args_bytes (multiple of 4, <= 1024) from args_src
   * (typically pinned HOST memory, read over PCIe) to args_dst (device) so that later kernels of
   * the same graph find the step's scalars in device memory without a separate copy node */
  const void* args_src;
  void* args_dst;
  int32_t args_bytes;
  /* > 0: dL/dlogits is scaled by this instead of 1/batch.  The exact full-data gradient
   * (inference_reject.py:18-33) is the sum over mega-batches of  -sum_i log p_i / N : scale = 1/N */
  float grad_scale;
  /* optional (else NULL): sgmcmc_mlp_split_scratch_floats(batch) floats of device scratch.  When
   * given, sgmcmc_dense_step_direct runs the forward/backward as TWO launches that spread the two
   * 784-wide contractions over 4x more workgroups (lower latency; same partial-gradient layout). */
  float* split_scratch;
} sgmcmc_mlp_args;

int64_t sgmcmc_mlp_split_scratch_floats(int batch);

int sgmcmc_mlp_fwdbwd(const sgmcmc_mlp_args* P, void* stream);
int64_t sgmcmc_mlp_lds_bytes(int in_features);

/* g <- sum_{s<n_slices} gpart[s*stride + noise_base_seg + j]  (fixed order)  - (1/N) dlog p/dtheta,
 * written to each segment's g; i.e. sgmcmc_prior_grad with the likelihood gradient taken from
 * per-slice partials (fp32 layouts only).  Also scalars[4] <- sum(loss_part)/batch,
 * scalars[5] <- sum(correct_part)/batch.  The log-density partials are produced when
 * (A_dev ? A_dev->flags : flags) has SGMCMC_CALC_METRICS and are finished by the following
 * sgmcmc_step* launch carrying SGMCMC_WITH_LOG_PRIOR. */
int sgmcmc_grad_reduce_prior(const sgmcmc_layout* L, const float* gpart, int n_slices,
                             int64_t stride, const float* loss_part, const float* correct_part,
                             int batch, double num_data, uint32_t flags,
                             const sgmcmc_step_args* A_dev, void* stream);

/* ---- native replay of the fused dense leapfrog step ------------------------------------- */
/* A "stepper" owns n_ring replicas of a hipGraph  mlp_fwdbwd -> step_indirect_parts (update +
 * finalize), captured on an internal stream at creation, one per pinned host slot.  One call to
 * sgmcmc_dense_stepper_step per leapfrog step: copies *A (per-step scalars) and idx[batch] (row
 * indices) into the next slot and launches that slot's replica on `stream`; the first kernel
 * reads the slot straight from host memory (row indices) and forwards the scalars to `dev_args`,
 * so there is no separate copy node.  A slot is reused only after the replay that read it has
 * completed (event wait): the host may run ahead of the GPU by up to n_ring steps.
 * Memory is the caller's: dev_args (device, >= sizeof(sgmcmc_step_args)), pinned (host-pinned,
 * n_ring*slot_bytes), slot_bytes >= sizeof(sgmcmc_step_args) + 8*batch and a multiple of 8;
 * mlp->idx and mlp->args_* are set per slot by the library. */
typedef struct sgmcmc_dense_stepper sgmcmc_dense_stepper;
int sgmcmc_dense_stepper_create(const sgmcmc_layout* L, const sgmcmc_mlp_args* mlp,
                                const sgmcmc_step_args* A_geometry, double num_data,
                                void* dev_args, void* pinned, int n_ring, int64_t slot_bytes,
                                sgmcmc_dense_stepper** out);
int sgmcmc_dense_stepper_step(sgmcmc_dense_stepper* S, const sgmcmc_step_args* A,
                              const int64_t* idx_host, void* stream);
int sgmcmc_dense_stepper_destroy(sgmcmc_dense_stepper* S);

/* The same leapfrog step as three DIRECT launches with every argument passed by value in
 * the kernel-argument segment -- including the minibatch's row indices (int32, batch <=
 * SGMCMC_MLP_MAX_INLINE) -- so there is no staging buffer, no copy and no graph: the runtime
 * snapshots the arguments at launch time.  mlp->idx / args_* are ignored. */
#define SGMCMC_MLP_MAX_INLINE 256
int sgmcmc_dense_step_direct(const sgmcmc_layout* L, const sgmcmc_mlp_args* mlp,
                             const sgmcmc_step_args* A, double num_data, const int64_t* idx_host,
                             const sgmcmc_step_args* A_pending, void* stream);
/* A_pending != NULL: the bookkeeping of an EARLIER transition launched with
 * SGMCMC_DEFER_FINALIZE (small-finalize layouts only) is executed by one extra workgroup of this
 * call's gradient kernel, i.e. concurrently with the forward/backward and before this call's
 * update kernel.  If A->flags has SGMCMC_DEFER_FINALIZE this call's own bookkeeping is left
 * pending in turn; otherwise it is launched as usual. */

/* The same three launches for SEVERAL independent chains at once (grid dimension y = chain): chains of one
 * architecture and one schedule, stepped in lock-step, each with its own weights, data order, sampler arena and
 * Philox stream (chain_id).  `chains_dev`: device array [n_chains], written once by the caller; `chain0_host`: a
 * host copy of element 0 (launch geometry); A: the transition's scalars, common to all chains (A->stream is
 * ignored: every chain draws from ITS stream; A must carry SMALL_FINALIZE and DEFER_FINALIZE); idx_host:
 * [n_chains][batch] data-set rows (16-bit: data sets of up to 65,536 rows); A_pending as sgmcmc_dense_step_direct.
 * Chain c's results are bit-identical to the same chain stepped alone by sgmcmc_dense_step_direct. */
#define SGMCMC_MAX_CHAINS 8
#define SGMCMC_MLP_BATCH_MULTI 128
typedef struct {
  sgmcmc_mlp_args mlp;
  sgmcmc_layout layout;
  double num_data;
  uint32_t chain_id, reserved;
} sgmcmc_dense_chain;
int sgmcmc_dense_step_multi(const sgmcmc_dense_chain* chains_dev, const sgmcmc_dense_chain* chain0_host, int n_chains,
                            const sgmcmc_step_args* A, const uint16_t* idx_host, const sgmcmc_step_args* A_pending,
                            void* stream);
/* The same for chains that do NOT share a schedule (a temperature ladder, a sweep over step sizes): where
 * sgmcmc_dense_step_multi takes ONE block of scalars for all chains, this takes `A`: [n_chains] blocks and `A_pending`:
 * [n_chains] blocks (or NULL), chain c stepping with A[c] and finalizing A_pending[c]; both arrays travel by value in
 * the kernel arguments (8 x 128 B).  Per chain: num_data, b2h2, bh, bhn, mom_decay, grad_v, noise_std (0 = that chain
 * does not draw), rmsprop_alpha, grad_clamp, seed.  One per launch -- hipErrorInvalidValue otherwise, checked on the
 * host before anything is launched: kind, flags, the segment and chunk ranges and draw, of A and of A_pending (chains
 * in lock-step share the sweep counter and the metric cadence).  A[c].stream is ignored as above.  Chain c's results
 * are bit-identical to the same chain stepped alone. */
int sgmcmc_dense_step_multi_args(const sgmcmc_dense_chain* chains_dev, const sgmcmc_dense_chain* chain0_host,
                                 int n_chains, const sgmcmc_step_args* A, const uint16_t* idx_host,
                                 const sgmcmc_step_args* A_pending, void* stream);

/* The per-segment bookkeeping of a transition that was launched with SGMCMC_DEFER_FINALIZE. */
int sgmcmc_finalize(const sgmcmc_layout* L, const sgmcmc_step_args* A, void* stream);

/* acc[j] <- (first ? 0 : acc[j]) + sum_{s<n_slices} gpart[s*stride + j]   for j < n  (fp64
 * accumulator, fixed order); out_f32[j] <- (float)acc[j] when out_f32 != NULL;
 * stats[0] += sum loss_part, stats[1] += sum correct_part (zeroed first when `first`).
 * Accumulates the mega-batches of the exact full-data gradient pass. */
int sgmcmc_accumulate_parts(const float* gpart, int n_slices, int64_t stride, double* acc,
                            float* out_f32, int64_t n, const float* loss_part,
                            const float* correct_part, double* stats, int first, void* stream);

/* 3x3, stride 1, zero-pad 1 convolution of the ResNet trunk on the fp32 matrix pipe, NCHW fp32,
 * `channels` -> `channels` (16 @ 32x32, 32 @ 16x16, 64 @ 8x8; anything else: hipErrorInvalidValue
 * and the caller keeps the shape on its library path).  Replaces the convolution inside
 * autograd's forward / backward of R1 (inference.py:215-223; models/google_resnet.py:34-43):
 *   transpose_w = 0:  y[n,co,p]  = sum_{ci,r,s} x[n,ci,p+(r-1,s-1)] w[co,ci,r,s]      (forward)
 *   transpose_w = 1:  y[n,ci,p]  = sum_{co,r,s} x[n,co,p-(r-1,s-1)] w[co,ci,r,s]      (data gradient,
 *                     x = the gradient w.r.t. the forward output)
 *   stats (forward only, may be NULL): [channels][sgmcmc_conv3x3_stat_slices(...)][2] doubles, the
 *   per-band (sum y, sum (y - band mean)^2) of every output channel -- the batch statistics of the BatchNorm that
 *   follows, taken from the accumulators (pass them to sgmcmc_bn_train_fwd as stats_in). */
int sgmcmc_conv3x3_stat_slices(int n_img, int channels, int hw);
int sgmcmc_conv3x3(const float* x, const float* w, float* y, int n_img, int channels, int hw,
                   int transpose_w, double* stats, void* stream);

/* Weight gradient of the same convolution: dw[co,ci,r,s] = sum_{n,p} dy[n,co,p] x[n,ci,p+(r-1,s-1)].
 * `scratch` holds sgmcmc_conv3x3_wrw_scratch_floats(...) floats of per-workgroup partial slabs that a
 * second launch sums in a fixed order (deterministic; no atomics).  -1 / hipErrorInvalidValue for
 * shapes outside the table above. */
int64_t sgmcmc_conv3x3_wrw_scratch_floats(int n_img, int channels, int hw);
int sgmcmc_conv3x3_wrw(const float* x, const float* dy, float* dw, float* scratch, int n_img,
                       int channels, int hw, void* stream);
/* Evaluation mode: y = relu?(BatchNorm_eval(conv3x3(x, w)) [+ residual]) in ONE launch -- with running statistics the
 * BatchNorm that follows a convolution is a per-channel affine map, applied to the accumulator tile in the epilogue
 * (invstd = 1 / sqrtf(var + eps); ((v - mean) * invstd) * gamma + beta; + residual; ReLU: sgmcmc_bn_eval_fwd's
 * arithmetic on sgmcmc_conv3x3's output, the same bits as the two launches).  Replaces conv -> BatchNorm2d.eval() ->
 * (+ shortcut) -> ReLU of models/google_resnet.py:34-56 inside the test-set passes (inference.py:199-213,
 * exp_utils.py:250-340).  residual may be NULL; the three trunk shapes. */
int sgmcmc_conv3x3_bn_eval(const float* x, const float* w, const float* gamma, const float* beta,
                           const float* running_mean, const float* running_var, double eps, const float* residual,
                           int relu, float* y, int n_img, int channels, int hw, void* stream);
/* Both gradients in one launch (they are independent and share the GPU): dx as sgmcmc_conv3x3 with
 * transpose_w = 1 on dy, dw and scratch as sgmcmc_conv3x3_wrw.  Results are bit-identical to the two
 * separate calls.
 * With `deferred_slabs` != NULL the slab reduction is NOT launched: *deferred_slabs receives the number of
 * slabs in `scratch` and the caller sums them later -- typically all weight gradients of a backward pass
 * in ONE launch of sgmcmc_wrw_reduce_many (same summation order: same bits). */
#define SGMCMC_REDUCE_JOBS 32
typedef struct sgmcmc_reduce_job {
  const float* part; /* [n_slabs][numel] */
  float* out;        /* [numel] */
  int32_t n_slabs, numel;
  int32_t taps;      /* <= 1: out[j] = sum_p part[p][j].  > 1: the slabs are TAP-MAJOR ([taps][numel / taps], what the 3x3
                      * weight-gradient kernels write: coalesced) and out is [numel / taps][taps] = [co][ci][r,s] */
  int32_t reserved;
} sgmcmc_reduce_job;
int sgmcmc_conv3x3_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw,
                       float* scratch, int n_img, int channels, int hw, int* deferred_slabs, void* stream);
/* ... with dx += e_dout * [e_out > 0] in the data gradient's epilogue: the gradient a residual block's identity
 * shortcut carries back to the block input (models/google_resnet.py:52-56: out = relu(bn2(conv2(h)) + x)), added where
 * the first convolution's data gradient is produced instead of by a separate element-wise pass. */
int sgmcmc_conv3x3_bwd_add(const float* x, const float* w, const float* dy, float* dx, const float* e_dout,
                           const float* e_out, float* dw, float* scratch, int n_img, int channels, int hw,
                           int* deferred_slabs, void* stream);
/* The general form: the data gradient's epilogue may add the shortcut's gradient (e_dout masked by [e_out > 0]; e_out NULL: e_dout as it is -- see mask_dx)
 * and / or leave the partial sums of the BatchNorm backward that CONSUMES dx as its incoming gradient (s_*: that
 * BatchNorm's input y, its post-ReLU output, its saved mean / invstd): s_partial[(c * S + slice) * 2 + {0,1}] =
 * sum dz, sum dz * xhat over the slice, dz = dx * [s_out > 0], xhat = (s_y - mean_c) * invstd_c, S =
 * sgmcmc_conv3x3_stat_slices(n_img, channels, hw) slices per channel -- what sgmcmc_bn_bwd_sums would compute in a
 * launch of its own (same quantities, another summation grouping); feed them to sgmcmc_bn_bwd_dx.
 * Replaces BatchNorm2d's backward reductions (models/google_resnet.py:34-43 inside inference.py:215-223). */
typedef struct {
  const float *e_dout, *e_out;
  const float *s_y, *s_out, *s_mean, *s_invstd;
  double* s_partial;
  int32_t group_imgs; /* > 0: the launch carries groups of this many images (sgmcmc_bn_train_fwd, GROUPS) and s_mean /
                       * s_invstd are [groups][channels]; 0: one batch */
  int32_t wrw_mult;   /* sgmcmc_conv3x3_bwd_ex only; > 1: every weight-gradient workgroup sums over wrw_mult times as many
                       * (image, band) items, i.e. *deferred_slabs shrinks by that factor -- for launches that carry
                       * several minibatches (the slab count of ONE minibatch, each slab the sum over more images;
                       * another summation grouping than wrw_mult = 1: equal to rounding); 0 / 1: the default */
  int32_t mask_dx;    /* with s_partial: dx is STORED as dz = dx * [s_out > 0].  Everything that consumes the gradient of a
                       * BatchNorm + ReLU output forms exactly that from it (the BatchNorm's own backward; the shortcut add
                       * of the residual block before), so neither has to read s_out again: feed such a dx to
                       * sgmcmc_bn_bwd_dx with relu = 0 (y unused) and as e_dout with e_out = NULL (added as it is).
                       * Same bits as masking at the consumers. */
  int32_t reserved;
} sgmcmc_conv_bwd_epilogue;
int sgmcmc_conv3x3_bwd_ex(const float* x, const float* w, const float* dy, float* dx,
                          const sgmcmc_conv_bwd_epilogue* epi, float* dw, float* scratch, int n_img, int channels,
                          int hw, int* deferred_slabs, void* stream);
int sgmcmc_wrw_reduce_many(const sgmcmc_reduce_job* jobs, int n_jobs, void* stream);
/* sgmcmc_conv3x3_bwd_ex whose launch ALSO reduces the slabs of up to SGMCMC_RIDE_JOBS earlier launches (`jobs`, as for
 * sgmcmc_wrw_reduce_many: the same blocks, the same bits) in a few extra workgroups -- riders.  Every job's slabs must
 * have been written by work enqueued EARLIER on `stream`: the kernel boundary is the only synchronisation.  The
 * reductions leave the dependent chain of a backward pass: a rider waits for memory in a workgroup slot that the
 * launch's own roles have no use for.  n_jobs = 0 is sgmcmc_conv3x3_bwd_ex.  riders_first != 0: the riders lead the grid
 * (padded to 8 blocks) instead of trailing it; the other workgroups run where they run without riders either way. */
#define SGMCMC_RIDE_JOBS 4
int sgmcmc_conv3x3_bwd_ride(const float* x, const float* w, const float* dy, float* dx,
                            const sgmcmc_conv_bwd_epilogue* epi, float* dw, float* scratch, int n_img, int channels,
                            int hw, int* deferred_slabs, const sgmcmc_reduce_job* jobs, int n_jobs, int riders_first,
                            void* stream);

#define SGMCMC_FRAG_JOBS 24   /* convolutions per launch of sgmcmc_conv3x3_prepare_weights */
/* ---- the same three contractions, PERSISTENT kernels on prepared weight fragments (csrc/conv2_hip.inc; round 3) ----
 * Replaces the convolutions of models/google_resnet.py:11-43 inside a gradient evaluation, as sgmcmc_conv3x3 /
 * sgmcmc_conv3x3_bwd_ex do, for the same three shapes.  WHERE THEY RUN: launches that carry several minibatches -- the
 * grouped exact full-data pass (inference_reject.py:18-33; graphed.py), 512 and more images per launch with the SAME
 * weights for a whole pass -- where persistent, double-buffered workgroups are 10-20 % faster (tools/conv_lab at 512
 * images: backward 62 -> 51 us at 32 channels, 65 -> 51 us at 64; forward 35 -> 28 us at 64; the pass 190 -> 172 ms).
 * The 128-image leapfrog step keeps sgmcmc_conv3x3[_bwd_ex] (there these are slower: 1,131 vs 1,154 steps/s,
 * DESIGN.md section 3).  Differences:
 *   - the weights are read as MFMA fragments that sgmcmc_conv3x3_prepare_weights leaves in caller-owned buffers of
 *     channels^2 * 9 floats each (forward order and transposed + flipped for the data gradient): ONE launch for all
 *     convolutions of a gradient evaluation (up to SGMCMC_FRAG_JOBS per launch; more are split over launches);
 *   - items of 4 image rows; workgroups are persistent over a stream of items, XCD-aware (an image's items, its
 *     channel tiles and both of its gradients are processed on XCD = image mod 8);
 *   - statistics / backward-sum partials: [channels][sgmcmc_conv3x3_frag_stat_slices(...)][2] doubles, slice =
 *     image * (hw / 4) + band -- equal parts, as sgmcmc_bn_train_fwd / sgmcmc_bn_bwd_dx expect;
 *   - weight-gradient slabs: `scratch` = [channels / 16][P][9][16][channels] floats, P = *deferred_slabs: one reduction
 *     job PER 16-output-channel tile t (part = scratch + t * P * 144 * channels, out = dw + t * 144 * channels,
 *     numel = 144 * channels, taps = 9).  With dw != NULL and deferred_slabs == NULL the reductions are launched here.
 * Results agree with the round-2 kernels up to fp32 summation order; runs are bitwise reproducible. */
typedef struct sgmcmc_frag_job {
  const float* w;  /* [channels][channels][3][3] */
  float* fwd;      /* channels^2 * 9 floats, or NULL */
  float* dgrad;    /* channels^2 * 9 floats, or NULL */
  int32_t channels, reserved;
} sgmcmc_frag_job;
int sgmcmc_conv3x3_prepare_weights(const sgmcmc_frag_job* jobs, int n_jobs, void* stream);
int sgmcmc_conv3x3_frag_stat_slices(int n_img, int channels, int hw);
int64_t sgmcmc_conv3x3_frag_scratch_floats(int n_img, int channels, int hw);
int sgmcmc_conv3x3_frag_fwd(const float* x, const float* frag_fwd, float* y, int n_img, int channels, int hw,
                            double* stats, void* stream);
int sgmcmc_conv3x3_frag_bwd(const float* x, const float* frag_dgrad, const float* dy, float* dx,
                            const sgmcmc_conv_bwd_epilogue* epi, float* dw, float* scratch, int n_img, int channels,
                            int hw, int* deferred_slabs, void* stream);
/* ---- sgmcmc_conv3x3 / sgmcmc_conv3x3_bwd_ride themselves on those fragments (csrc/conv_hip.inc, FRAG) ----
 * The default kernels of the 128-image step -- same tiling, same statistics slices, same slabs, same MFMA order, hence
 * the SAME BITS as the raw-weight entry points -- whose workgroups read their B operands from the fragments of
 * sgmcmc_conv3x3_prepare_weights (or of sgmcmc_conv_stem_fwd_frags, which prepares them without a launch) instead of
 * each permuting the raw [co][ci][3][3] tensor.  form: 1 = the tile's fragments are copied to LDS linearly and read back
 * 16 bytes per lane; 2 = 16-byte global loads straight into the operand registers, no weight slab in LDS.
 * sgmcmc_conv3x3_wfrag_fwd: sgmcmc_conv3x3 with transpose_w = 0 and stats (required), on frag_fwd.
 * sgmcmc_conv3x3_wfrag_bwd: sgmcmc_conv3x3_bwd_ride (n_jobs = 0: sgmcmc_conv3x3_bwd_ex) on frag_dgrad, for the
 * epilogues of the leapfrog step only: s_partial is required (with or without e_dout), wrw_mult must be 0 or 1. */
int sgmcmc_conv3x3_wfrag_fwd(const float* x, const float* frag_fwd, float* y, int n_img, int channels, int hw,
                             double* stats, int form, void* stream);
int sgmcmc_conv3x3_wfrag_bwd(const float* x, const float* frag_dgrad, const float* dy, float* dx,
                             const sgmcmc_conv_bwd_epilogue* epi, float* dw, float* scratch, int n_img, int channels,
                             int hw, int* deferred_slabs, const sgmcmc_reduce_job* jobs, int n_jobs, int riders_first,
                             int form, void* stream);


/* The two convolutions that open a down-sampling ResNet block, as one operator (they read the same input;
 * the 1x1 shortcut's operand is the 3x3's centre tap): models/google_resnet.py:77-90.
 *   y_main[n,co,oy,ox]  = sum_{ci,r,s} x[n,ci,2oy+r-1,2ox+s-1] w_main[co,ci,r,s]     (3x3, stride 2, pad 1)
 *   y_short[n,co,oy,ox] = sum_ci x[n,ci,2oy,2ox] w_short[co,ci]                        (1x1, stride 2)
 * cin -> 2 cin channels, hwi -> hwi/2 pixels, for (cin, hwi) = (16, 32) and (32, 16).  stats_main /
 * stats_short (both or neither): [2 cin][sgmcmc_conv_down_stat_slices(...)][2] per-band (sum, centred sum
 * of squares) of the two outputs, as for sgmcmc_conv3x3. */
int sgmcmc_conv_down_stat_slices(int n_img, int cin, int hwi);
int sgmcmc_conv_down_fwd(const float* x, const float* w_main, const float* w_short, float* y_main,
                         float* y_short, double* stats_main, double* stats_short, int n_img, int cin,
                         int hwi, void* stream);
/* All three gradients in one launch: dx (both paths summed: the transposed convolutions, evaluated per
 * parity class of the input pixel so that no multiply is spent on zeros), dw_main, dw_short.  `scratch`:
 * sgmcmc_conv_down_scratch_floats(...) floats, laid out [n_slabs][18 cin^2] then [n_slabs][2 cin^2];
 * `deferred_slabs` as for sgmcmc_conv3x3_bwd (two jobs for sgmcmc_wrw_reduce_many). */
int64_t sgmcmc_conv_down_scratch_floats(int n_img, int cin, int hwi);
int sgmcmc_conv_down_bwd(const float* x, const float* w_main, const float* w_short, const float* dy_main,
                         const float* dy_short, float* dx, float* dw_main, float* dw_short, float* scratch,
                         int n_img, int cin, int hwi, int* deferred_slabs, void* stream);
/* ... with the SUMS half of sgmcmc_conv_bwd_epilogue (e_dout / e_out must be NULL): the partial sums of the BatchNorm
 * backward whose incoming gradient dx is, [cin][sgmcmc_conv_down_bwd_sum_slices(...)][2] doubles. */
int sgmcmc_conv_down_bwd_sum_slices(int n_img, int cin, int hwi);
int sgmcmc_conv_down_bwd_ex(const float* x, const float* w_main, const float* w_short, const float* dy_main,
                            const float* dy_short, float* dx, const sgmcmc_conv_bwd_epilogue* epi, float* dw_main,
                            float* dw_short, float* scratch, int n_img, int cin, int hwi, int* deferred_slabs,
                            void* stream);

/* The stem convolution, 3 -> 16 channels, 3x3 / stride 1 / pad 1 on 32x32 images (google_resnet.py:96-100):
 * forward (+ optional per-band statistics [16][4 n_img][2]) and weight gradient (the images take no
 * gradient); scratch / deferred_slabs as for sgmcmc_conv3x3_bwd. */
int sgmcmc_conv_stem_fwd(const float* x, const float* w, float* y, double* stats, int n_img, void* stream);
/* ... as the carrier of the trunk's weight fragments: the stem is the first launch of a gradient evaluation and reads no
 * trunk weight, so n_jobs <= SGMCMC_FRAG_JOBS jobs of sgmcmc_conv3x3_prepare_weights (the same buffers, the same
 * values) are done by workgroups that trail its grid -- no launch of their own.  Consumers must be enqueued later on
 * `stream`.  n_jobs = 0 is sgmcmc_conv_stem_fwd.  jobs_first != 0: those workgroups lead the grid (padded to 8 blocks)
 * instead of trailing it. */
int sgmcmc_conv_stem_fwd_frags(const float* x, const float* w, float* y, double* stats, int n_img,
                               const sgmcmc_frag_job* jobs, int n_jobs, int jobs_first, void* stream);
int64_t sgmcmc_conv_stem_scratch_floats(int n_img);
int sgmcmc_conv_stem_wrw(const float* x, const float* dy, float* dw, float* scratch, int n_img,
                         int* deferred_slabs, void* stream);

/* The convolutional classifier's first layer (models/conv_nets.py:44-51): 1 -> 50 channels, 3x3 / stride 1 /
 * pad 1 on 28x28 images, without its bias (see sgmcmc_bias_relu_pool_*): forward and weight gradient
 * (n_img slabs of 450 floats; scratch / deferred_slabs as for sgmcmc_conv3x3_bwd). */
int sgmcmc_conv_first_fwd(const float* x, const float* w, float* y, int n_img, void* stream);
int64_t sgmcmc_conv_first_scratch_floats(int n_img);
int sgmcmc_conv_first_wrw(const float* x, const float* dy, float* dw, float* scratch, int n_img,
                          int* deferred_slabs, void* stream);
/* ... and the layer WITH its tail, Conv2d(1, 50, 3, padding=1) -> + bias -> ReLU -> MaxPool2d(2)
 * (models/conv_nets.py:46-57), one launch each way; the 50 x 28 x 28 map is never written.
 *   fwd: pooled [n][50][14][14] and code [n][50][14][14] bytes -- bits 0-1 the window position of the first maximum
 *        in scan order (NaNs win, as ATen's max_pool2d), bit 2 set when max + bias > 0.
 *   bwd: from the gradient w.r.t. pooled and code: weight-gradient slabs [P][450] at scratch and, with want_bias,
 *        bias-gradient slabs [P][50] behind them (P = 7 n_img bands); reduced into dw / dbias here, or --
 *        deferred_slabs != NULL -- *deferred_slabs = P and the caller runs sgmcmc_wrw_reduce_many over both. */
int sgmcmc_conv_first_pool_fwd(const float* x, const float* w, const float* bias, float* pooled, uint8_t* code,
                               int n_img, void* stream);
int64_t sgmcmc_conv_first_pool_scratch_floats(int n_img);
int sgmcmc_conv_first_pool_bwd(const float* x, const float* dpooled, const uint8_t* code, float* dw, float* dbias,
                               float* scratch, int n_img, int want_bias, int* deferred_slabs, void* stream);

/* The convolutional classifier's SECOND convolution (models/conv_nets.py:46-70): 50 -> 50 channels, 3x3 / stride 1 /
 * pad 1 on 14x14 maps, without its bias (see sgmcmc_bias_relu_pool_*), on the fp32 matrix pipe (csrc/conv50_hip.inc).
 *   sgmcmc_conv50: transpose_w = 0 forward, 1 data gradient (x = the gradient w.r.t. the forward output);
 *   sgmcmc_conv50_bwd: data gradient (dx may be NULL: weight gradient only) and weight gradient in one launch;
 *     scratch: sgmcmc_conv50_scratch_floats(n_img) floats of partial slabs; deferred_slabs as sgmcmc_conv3x3_bwd. */
int sgmcmc_conv50(const float* x, const float* w, float* y, int n_img, int transpose_w, void* stream);
int64_t sgmcmc_conv50_scratch_floats(int n_img);
int sgmcmc_conv50_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* scratch, int n_img,
                      int* deferred_slabs, void* stream);
/* Round 3: the forward also leaves wT[ci][co][rs] = w[co][ci][8 - rs] (2500 * 9 floats; NULL: not wanted) -- the weights
 * as the data gradient's rows -- so that the backward stages them with the forward's straight copy instead of strided
 * gathers: sgmcmc_conv50_bwd_t(x, wT, dy, dx (required), dw, scratch, ...) = sgmcmc_conv50_bwd with w replaced by the
 * wT of a forward on the SAME weights; a data gradient alone is sgmcmc_conv50_fwd(dy, wT, dx, NULL, ...). */
int sgmcmc_conv50_fwd(const float* x, const float* w, float* y, float* wT, int n_img, void* stream);
int sgmcmc_conv50_bwd_t(const float* x, const float* wT, const float* dy, float* dx, float* dw, float* scratch,
                        int n_img, int* deferred_slabs, void* stream);
/* ... and the layer WITH its tail, Conv2d(50, 50, 3, padding=1) -> + bias -> ReLU -> MaxPool2d(2)
 * (models/conv_nets.py:58-66), one launch each way; the 50 x 14 x 14 map and its gradient exist in LDS only.
 *   fwd: pooled [n][50][7][7], code [n][50][7][7] bytes (encoding of sgmcmc_conv_first_pool_fwd), wT as
 *        sgmcmc_conv50_fwd (may be NULL).
 *   bwd: from the gradient w.r.t. pooled and code: dx [n][50][14][14] (required), weight-gradient slabs [P][22500]
 *        (tap-major) at scratch and, with want_bias, bias-gradient slabs [P][50] behind them (P = ceil(n_img / 2));
 *        reduced into dw / dbias here, or -- deferred_slabs != NULL -- left to sgmcmc_wrw_reduce_many. */
int sgmcmc_conv50_pool_fwd(const float* x, const float* w, const float* bias, float* pooled, uint8_t* code, float* wT,
                           int n_img, void* stream);
int64_t sgmcmc_conv50_pool_scratch_floats(int n_img);
int sgmcmc_conv50_pool_bwd(const float* x, const float* wT, const float* dpooled, const uint8_t* code, float* dx,
                           float* dw, float* dbias, float* scratch, int n_img, int want_bias, int* deferred_slabs,
                           void* stream);

/* Training-mode batch normalisation over (N, H*W) per channel of an NCHW fp32 tensor, fused with the
 * optional residual add and ReLU that follow it in the ResNet trunk (models/google_resnet.py:34-43,
 * 77-90; replaces nn.BatchNorm2d + `+ shortcut` + ReLU inside R1's autograd graph):
 *   y = relu?(gamma * (x - mean) * invstd + beta [+ residual]);  save_mean / save_invstd are
 *   written for the backward; running_mean / running_var (both or neither) get nn.BatchNorm2d's momentum
 *   update with the unbiased batch variance.  `plane` = H*W must be a multiple of 4.
 * Backward: dz = dy * (y > 0) when relu;  dresidual (optional) = dz;  dbeta = sum dz;
 *   dgamma = sum dz * xhat;  dx = gamma * invstd * (dz - dbeta/M - xhat * dgamma/M).
 * `scratch`: sgmcmc_bn_scratch_doubles(n, channels, plane, groups) doubles of per-slice partial sums, combined in
 * a fixed order (deterministic).  Forward: when `stats_in` ([channels][stats_slices][2] partial (sum, sum of squared
 * deviations from the partial's own mean) of x over EQUAL parts, e.g. from sgmcmc_conv3x3) is given, the statistics
 * pass over x is skipped.
 *
 * GROUPS (round 4).  `groups` = G >= 1 independent minibatches of n / G images each, stored one after the other, in ONE
 * launch: the exact full-data gradient (inference_reject.py:18-33) evaluates its minibatches several per launch chain,
 * and training-mode statistics are per minibatch (models/google_resnet.py:14-27).  Every group is normalised with its
 * own batch statistics and gives the bits of a launch on that group alone:
 *   - `n`, `stats_slices`, `n_partials` count the WHOLE launch (multiples of G); a producer's image-major partials
 *     ([channels][slices][2] from the convolutions' epilogues) are read as [channels][G][slices / G][2];
 *   - save_mean / save_invstd: [G][channels];  dgb: [G][2][channels] = every group's (dgamma, dbeta) -- a caller whose
 *     parameters are shared by the groups sums the G rows (sgmcmc_wrw_reduce_many: n_slabs = G, numel = 2 channels);
 *   - stat_log: group g's row at stat_log + g * log_stride doubles;
 *   - running statistics cannot be advanced in place when G > 1 (the groups' updates are ordered): pass NULL or use
 *     the logging entry point; hipErrorInvalidValue otherwise.
 * gamma / beta are shared by the groups. */
/* Evaluation mode (model.eval(): the per-epoch posterior-predictive evaluation of inference.py:199-213): one pass with
 * the running statistics, y = relu?(gamma (x - running_mean) / sqrt(running_var + eps) + beta [+ residual]). */
int sgmcmc_bn_eval_fwd(const float* x, const float* residual, const float* gamma, const float* beta,
                       const float* running_mean, const float* running_var, double eps, int relu, int n,
                       int channels, int plane, float* y, void* stream);
int64_t sgmcmc_bn_scratch_doubles(int n, int channels, int plane, int groups);
int sgmcmc_bn_train_fwd(const float* x, const float* residual, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, double momentum, double eps, int relu,
                        int n, int channels, int plane, float* y, float* save_mean, float* save_invstd,
                        double* scratch, const double* stats_in, int stats_slices, int groups, void* stream);
/* The same forward with the running statistics left ALONE: the batch mean and unbiased variance of every channel go to
 * stat_log[2 c + {0,1}] (doubles; group g: + g * log_stride) instead, and sgmcmc_bn_running_replay advances
 * running_mean / running_var by a sequence of such entries (log + j * entry_stride doubles, j = 0 .. n_entries - 1) in
 * order -- the same bits as n_entries forwards in that order.  For gradient passes whose minibatches are evaluated
 * concurrently -- on several streams and / or several per launch (the exact full-data pass, inference_reject.py:18-33)
 * -- while nn.BatchNorm2d's running statistics must still advance batch by batch. */
int sgmcmc_bn_train_fwd_log(const float* x, const float* residual, const float* gamma, const float* beta,
                            double* stat_log, int64_t log_stride, double eps, int relu, int n, int channels, int plane,
                            float* y, float* save_mean, float* save_invstd, double* scratch, const double* stats_in,
                            int stats_slices, int groups, void* stream);
int sgmcmc_bn_running_replay(const double* log, int64_t entry_stride, int n_entries, double momentum,
                             float* running_mean, float* running_var, int channels, void* stream);
/* ... for all BatchNorm layers of a network in ONE launch (any number: SGMCMC_BN_REPLAY_LAYERS per launch): layer i's
 * entries are layers[i].log + j * entry_stride (the layers' columns of one log array). */
#define SGMCMC_BN_REPLAY_LAYERS 32
typedef struct sgmcmc_bn_replay_layer {
  const double* log;
  float *running_mean, *running_var;
  double momentum;
  int32_t channels, reserved;
} sgmcmc_bn_replay_layer;
int sgmcmc_bn_running_replay_many(const sgmcmc_bn_replay_layer* layers, int n_layers, int64_t entry_stride,
                                  int n_entries, void* stream);
int sgmcmc_bn_train_bwd(const float* dy, const float* y, const float* x, const float* gamma,
                        const float* save_mean, const float* save_invstd, int relu, int n, int channels,
                        int plane, float* dx, float* dresidual, float* dgb, double* scratch, int groups, void* stream);
/* The first launch of sgmcmc_bn_train_bwd (relu = 1) on its own: per-slice partial sums of dz = dout * [out > 0] and
 * dz * xhat, sums [channels][*n_sums][2] doubles (sgmcmc_bn_scratch_doubles(...) of them; *n_sums counts all groups). */
int sgmcmc_bn_bwd_sums(const float* dout, const float* out, const float* y, const float* save_mean,
                       const float* save_invstd, double* sums, int* n_sums, int n, int channels, int plane,
                       int groups, void* stream);
/* The second launch of sgmcmc_bn_train_bwd alone, for partial sums that already exist: `partial` =
 * [channels][n_partials][2] doubles (sum dz, sum dz * xhat per slice) from sgmcmc_bn_bwd_sums or from the epilogue of
 * the convolution gradient that produced dy (sgmcmc_conv3x3_bwd_ex).
 * rs (may be NULL): the residual is itself the output of a BatchNorm WITHOUT ReLU (the down-sampling block's shortcut,
 * models/google_resnet.py:77-90) whose incoming gradient is dresidual = dz -- with relu: formed here and stored
 * (dresidual required); with relu = 0: dy arrives masked already (sgmcmc_conv_bwd_epilogue.mask_dx), the residual's
 * gradient IS dy and dresidual must be NULL; the launch
 * also leaves that BatchNorm's backward sums in rs->partial, [channels][sgmcmc_bn_scratch_doubles(...) / (2
 * channels)][2] doubles (the slices of this launch's own geometry); rs->mean / rs->invstd: [G][channels]. */
typedef struct {
  const float *y, *mean, *invstd; /* the residual BatchNorm's input and saved statistics */
  double* partial;
} sgmcmc_bn_residual_sums;
int sgmcmc_bn_bwd_dx(const float* dy, const float* y, const float* x, const float* gamma, const float* save_mean,
                     const float* save_invstd, int relu, int n, int channels, int plane, const double* partial,
                     int n_partials, float* dx, float* dresidual, float* dgb, const sgmcmc_bn_residual_sums* rs,
                     int groups, void* stream);
/* out = relu(BN(x) + BN_s(r)): a down-sampling block's last BatchNorm (models/google_resnet.py:77-90) with the 1x1
 * shortcut's BatchNorm -- no ReLU, this sum its only consumer -- applied on the fly: the shortcut BatchNorm's own
 * launch and its output tensor disappear; the same bits as sgmcmc_bn_train_fwd twice.  Training mode; both layers'
 * batch statistics as equal-part partial pairs [channels][slices][2] (a convolution epilogue's); save_* / running_* /
 * stat_log (+ log_stride) per layer as for sgmcmc_bn_train_fwd[_log]. */
typedef struct {
  const float* r;     /* the shortcut BatchNorm's input */
  const float* gamma;
  const float* beta;
  const double* partial;
  int n_partials, reserved;
  double eps, momentum;
  float *save_mean, *save_invstd, *running_mean, *running_var;
  double* stat_log;
  int64_t log_stride;
} sgmcmc_bn_dual;
int sgmcmc_bn_train_fwd_dual(const float* x, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, double momentum, double eps, int n, int channels, int plane, float* y,
                             float* save_mean, float* save_invstd, const double* stats_in, int stats_slices,
                             double* stat_log, int64_t log_stride, const sgmcmc_bn_dual* rs, int groups, void* stream);

/* y = maxpool2x2(relu(x + bias_c)), NCHW fp32, h and w even: the Conv2d(+bias) -> ReLU -> MaxPool2d(2) tail
 * of models/conv_nets.py:44-56 in one pass (the convolution itself is then run without its bias).
 * Backward: dx in full (the gradient goes to the first maximal element of each window, as ATen, if its
 * pre-activation is positive); dbias_part (may be NULL): [sgmcmc_pool_slices(...)][channels] partial sums
 * for sgmcmc_wrw_reduce_many.  `bias` may be NULL (= 0). */
int sgmcmc_pool_slices(int n, int channels, int h, int w);
int sgmcmc_bias_relu_pool_fwd(const float* x, const float* bias, float* y, int n, int channels, int h, int w,
                              void* stream);
int sgmcmc_bias_relu_pool_bwd(const float* x, const float* bias, const float* dy, float* dx,
                              float* dbias_part, int n, int channels, int h, int w, void* stream);

/* The ResNet's classifier head (google_resnet.py:103-110: AvgPool2d over the whole map -> Flatten -> Linear):
 *   pooled[n,c] = mean_p h[n,c,p];  logits[n,k] = bias[k] + sum_c weight[k,c] pooled[n,c]
 * and its gradients: dh[n,c,p] = (sum_k dlogits[n,k] weight[k,c]) / plane; slab_w [n][classes*channels] and
 * slab_b [n][classes] (either may be NULL) are per-row terms of dweight / dbias for sgmcmc_wrw_reduce_many
 * (n slabs).  channels <= 64, plane a multiple of 16, classes <= 16; bias may be NULL. */
int sgmcmc_pool_linear_fwd(const float* h, const float* weight, const float* bias, float* pooled,
                           float* logits, int n, int channels, int plane, int classes, void* stream);
int sgmcmc_pool_linear_bwd(const float* dlogits, const float* pooled, const float* weight, float* dh,
                           float* slab_w, float* slab_b, int n, int channels, int plane, int classes,
                           void* stream);
/* The head, the softmax cross-entropy on its logits and both backward passes in ONE launch (round 3): everything
 * between the trunk's last activation h and its gradient dh is per image.  Outputs: pooled / logits as
 * sgmcmc_pool_linear_fwd, loss_rows[n] = -log softmax(logits_n)[y_n], dlogits = grad_scale * (softmax - onehot) -- the
 * bits of sgmcmc_softmax_xent_fwd_grad -- and dh / slab_w / slab_b (/ partial, with the four bn_* pointers: plane == 64)
 * as sgmcmc_pool_linear_bwd[_sums] would produce from that dlogits.  counters (may be NULL): n_counters <= 256 int64
 * values that get + 1 (the BatchNorm layers' num_batches_tracked, kept in one array).  A label outside [0, classes):
 * see "Labels" at sgmcmc_softmax_xent_fwd.  Replaces the head's Linear,
 * Categorical(logits).log_prob and their autograd backward inside R1 (inference.py:215-223, models/base.py:168-191). */
int sgmcmc_pool_linear_loss(const float* h, const float* weight, const float* bias, const int64_t* y, float* pooled,
                            float* logits, float* dlogits, float* loss_rows, float* dh, float* slab_w, float* slab_b,
                            const float* bn_y, const float* bn_out, const float* bn_mean, const float* bn_invstd,
                            double* partial, int group_rows, int64_t* counters, int n_counters, int n, int channels,
                            int plane, int classes, float grad_scale, void* stream);
/* ... when h is the output of a BatchNorm + ReLU (bn_y its input, bn_out = h, saved mean / invstd) on 8x8 maps
 * (plane == 64): the launch also leaves that BatchNorm's backward sums, partial[(c * n + image) * 2 + {0,1}] doubles
 * (n slices per channel) for sgmcmc_bn_bwd_dx -- the last BatchNorm of models/google_resnet.py:103-110's trunk.
 * group_rows > 0: that BatchNorm ran on groups of group_rows rows (sgmcmc_bn_train_fwd, GROUPS): bn_mean / bn_invstd are
 * [n / group_rows][channels]; 0: one batch. */
int sgmcmc_pool_linear_bwd_sums(const float* dlogits, const float* pooled, const float* weight, float* dh,
                                float* slab_w, float* slab_b, const float* bn_y, const float* bn_out,
                                const float* bn_mean, const float* bn_invstd, double* partial, int group_rows, int n,
                                int channels, int plane, int classes, void* stream);

/* A narrow linear layer, y = x W^T + b with out_features <= 16 (the convolutional classifier's head,
 * Flatten -> Linear(2450, 10), models/conv_nets.py:57-70): one launch each way, fixed-order reductions.
 * Backward, one launch: dx (may be NULL), dbias (may be NULL) and the weight gradient as
 * sgmcmc_linear_row_groups(n) partial slabs [group][out_features][in_features] (may be NULL), one per group of 16
 * batch rows, for sgmcmc_wrw_reduce_many (fixed order). */
int sgmcmc_linear_fwd(const float* x, const float* weight, const float* bias, float* y, int n, int in_features,
                      int out_features, void* stream);
/* sgmcmc_linear_fwd and, in the same launch, the rows' softmax cross-entropy on the logits it produced: dlogits =
 * grad_scale * (softmax(y_n) - onehot(y_labels[n])) and loss_rows[n] = -log softmax(y_n)[y_labels[n]] -- the bits of
 * sgmcmc_softmax_xent_fwd_grad (models/conv_nets.py:57-70 + models/base.py:168-191 in one launch).  A label outside
 * [0, out_features): see "Labels" at sgmcmc_softmax_xent_fwd. */
int sgmcmc_linear_fwd_loss(const float* x, const float* weight, const float* bias, const int64_t* y_labels, float* y,
                           float* dlogits, float* loss_rows, int n, int in_features, int out_features,
                           float grad_scale, void* stream);
int sgmcmc_linear_row_groups(int n);
int sgmcmc_linear_bwd(const float* x, const float* weight, const float* dy, float* dx, float* dweight_slabs,
                      float* dbias, int n, int in_features, int out_features, void* stream);

/* Minibatch gather from an HBM-resident image set with random crop (zero padding `pad`) and horizontal flip
 * applied on the way -- the `cifar10_augmented` pipeline (data/CIFAR/cifar.py:136-172: RandomCrop(32,
 * padding=4), RandomHorizontalFlip) without leaving the device:
 *   out[b,c,y,x] = data[idx[b], c, y + dy - pad, x' + dx - pad] (fill[c] outside; fill == NULL: 0),
 *   x' = flip_b ? W-1-x : x,
 *   (dx, dy, flip_b) = Philox4x32-10(seed; counter (idx[b], draw, purpose 3, stream)) -> r0 % (2 pad + 1),
 *   r1 % (2 pad + 1), r2 & 1 (only if `flip`).  `idx`: int64 device array of data-set rows; `draw`: the
 *   caller's per-pass counter.  pad = 0 and flip = 0 is a plain gather.  `fill` (device, [channels], or NULL):
 *   the value of the padding -- the reference pads the RAW image with black before normalising, so on
 *   normalised data the padding of channel c is (0 - mean_c) / std_c. */
int sgmcmc_augment_gather(const float* data, const int64_t* idx, float* out, const float* fill, int batch,
                          int channels, int height, int width, int pad, int flip, uint64_t seed,
                          uint32_t stream, uint64_t draw, void* stream_);

/* Round 4: everything between two replays of a captured step in ONE launch -- sgmcmc_augment_gather into `out` (the
 * graph's static input; pad = 0, flip = 0, channels = height = 1: a plain row gather), the labels gathered beside it
 * (labels_out[b] = labels[idx[b]]; both NULL: none), up to three plain copies as sgmcmc_stage_batch (the argument block
 * from its pinned slot; n_copies may be 0) and the previous transition's deferred bookkeeping (A_pending, as
 * sgmcmc_stage_batch).  Replaces the DataLoader hand-over of inference.py:197-205 + data/CIFAR/cifar.py:136-172 for a
 * captured step: 1 launch instead of 3 (gather, label index_select, staging copy). */
typedef struct sgmcmc_gather {
  const float* data;          /* [rows][channels][height][width] */
  const int64_t* labels;      /* [rows] or NULL */
  const int64_t* idx;         /* [batch] data-set rows */
  float* out;                 /* [batch][channels][height][width] */
  int64_t* labels_out;        /* [batch] or NULL */
  const float* fill;          /* [channels] or NULL */
  int32_t batch, channels, height, width, pad, flip;
  uint64_t seed, draw;
  uint32_t stream, reserved;
} sgmcmc_gather;
int sgmcmc_gather_stage(const sgmcmc_gather* G, const void* const* src, void* const* dst, const int64_t* bytes,
                        int n_copies, const sgmcmc_layout* L, const sgmcmc_step_args* A_pending, void* stream);

/* Up to three plain device copies in ONE launch: dst[j][0 .. bytes[j]) = src[j][...].  For the per-step staging of a
 * captured step -- the minibatch (x, y) into the graph's static inputs and the argument block from PINNED host
 * memory (the kernel reads it over the bus) -- which otherwise costs three copy dispatches between two graph
 * launches.  Pointers 16-byte aligned, sizes multiples of 4; else hipErrorInvalidValue.  No reference counterpart:
 * the reference's batches arrive from its DataLoader (experiments/train_bnn.py:172-180).
 * A_pending (may be NULL; else with L): the previous transition was launched with SGMCMC_DEFER_FINALIZE
 * (SMALL_FINALIZE layouts) and its per-segment bookkeeping is executed by extra workgroups of THIS launch -- the
 * same results as sgmcmc_finalize(L, A_pending) at this point of the stream. */
int sgmcmc_stage_batch(const void* const* src, void* const* dst, const int64_t* bytes, int n_copies,
                       const sgmcmc_layout* L, const sgmcmc_step_args* A_pending, void* stream);

/* loss = scale * sum_b -log softmax(logits_b)[y_b] for up to 1024 rows of up to 16 classes (the likelihood term of
 * models/base.py:168-191), one launch each way: forward keeps probs [rows][classes] for the backward,
 * dlogits = *grad_out * scale * (probs - onehot(y)).  scale = 1/rows for the minibatch mean, 1/N in the exact
 * full-data pass.
 *
 * Labels -- one rule for every entry point that takes the likelihood: sgmcmc_softmax_xent_fwd / _fwd_grad / _bwd,
 * sgmcmc_pool_linear_loss and sgmcmc_linear_fwd_loss (one device function, csrc/pool_hip.inc xent::row).  The int64
 * label is compared as 64 bits against [0, classes): nothing is truncated to 32 bits first.  A label outside that range
 * (an ignore index, a corrupt batch) gives its row a NaN loss -- so the total of sgmcmc_softmax_xent_fwd[_grad] is NaN --
 * and a gradient without the one-hot term, dlogits = grad_scale * softmax; every other row is what it would be beside a
 * valid label.  No address is formed from a label: x_t is selected by comparison, never read at an index, so no label
 * can make a launch read outside the logits.  (ATen raises a device-side assertion instead, which takes the whole
 * process's context with it.)  For labels inside the range the three routes give the same bits. */
int sgmcmc_softmax_xent_fwd(const float* logits, const int64_t* y, float* probs, float* loss, int rows,
                            int classes, double scale, void* stream);
int sgmcmc_softmax_xent_bwd(const float* probs, const int64_t* y, const float* grad_out, float* dlogits,
                            int rows, int classes, double scale, void* stream);
/* The same loss AND its gradient in one launch, for a caller that seeds autograd itself (logits.backward(dlogits)):
 * dlogits[b,k] = grad_scale * (softmax(logits_b)[k] - [k == y_b]) -- bit-identical to sgmcmc_softmax_xent_bwd on the
 * saved probabilities with grad_out[0] * scale == grad_scale. */
int sgmcmc_softmax_xent_fwd_grad(const float* logits, const int64_t* y, float* loss, float* dlogits, int rows,
                                 int classes, double scale, float grad_scale, void* stream);

/* ---- Calibration and out-of-distribution metrics of a posterior ensemble (evaluation, fp64, deterministic) -----------
 * The reference computes these in numpy on the host from the [E, N, C] tables (experiments/eval_bnn.py calibration_eval /
 * ood_eval -> exp_utils.py:323-327, 343-380, third_party/calibration_error.py).  Here the tables stay on the device and
 * only the final scalars are read back.  Sums run in an order fixed by the sizes; counts are integers. */
#define SGMCMC_CALIB_MAX_CLASSES 128
#define SGMCMC_CALIB_MAX_ROWS 131072
#define SGMCMC_CALIB_MAX_BINS 4096

/* exp_utils.py:309,324 (Categorical(logits=_log_space_mean(acc_data, 0)).probs) and the max-prob / argmax of
 * calibration_error.py:226-229: per row n of acc [samples][rows][classes] (normalised log-probabilities),
 * lme = logsumexp_e acc[e, n, :] - log(samples) summed over e in order, probs[n, :] = softmax(lme),
 * conf[n] = max_c probs[n, c], pred[n] = its first index (np.argmax), hit[n] = (pred[n] == labels[n]).
 * labels and hit: both NULL or both given.  classes <= SGMCMC_CALIB_MAX_CLASSES. */
int sgmcmc_ensemble_probs(const double* acc, const int64_t* labels, int samples, int rows, int classes, double* probs,
                          double* conf, int64_t* pred, int64_t* hit, void* stream);
/* The conf / pred / hit part of sgmcmc_ensemble_probs for given probabilities probs [rows][classes]. */
int sgmcmc_row_max(const double* probs, const int64_t* labels, int rows, int classes, double* conf, int64_t* pred,
                   int64_t* hit, void* stream);
/* np.argsort(kind="stable") of ncols independent columns (calibration_error.py:57 np.sort, sklearn's ranking):
 * column j's key i is keys[j * col_stride + i * elem_stride]; perm [ncols][n] (int32) receives, per column, the rows
 * in ascending order, ties by row.  -0.0 equals 0.0; NaN sorts after every number, as in numpy.
 * n <= SGMCMC_CALIB_MAX_ROWS.  One launch; every perm entry is written. */
int sgmcmc_stable_order(const double* keys, int64_t elem_stride, int64_t col_stride, int n, int ncols, int32_t* perm,
                        void* stream);
/* GeneralCalibrationError.get_calibration_error / update_state (calibration_error.py:173-195, 197-277) on columns
 * sorted by sgmcmc_stable_order (same keys, strides, n, ncols).  Per column j: the keys > 0; bins even (bounds:
 * num_bins upper bounds, np.histogram_bin_edges([], num_bins, (0, 1))[1:]) or adaptive (bounds NULL: num_bins bins,
 * upper bounds sorted[min(rint(i * (m / num_bins)), m - 1)], i = 1..num_bins-1, over the m kept keys; num_bins <= 1:
 * one bin); np.digitize's bins; per bin the count, the score sum and the hits, where row r counts as a hit if
 * target[r] == (class_conditional ? j : 1); err_j = sum_bins |(acc - conf) w| (l2: ((acc - conf) w)^2) with
 * conf = S / (cnt + eps), acc = H / (cnt + eps), w = (cnt + eps) / m, eps = 2^-52; err_j = 0 if m = 0, NaN if the
 * column holds a NaN.  col_err [ncols]: caller workspace.  out[0] = class_conditional ? sum_j err_j / ncols : err_0,
 * square-rooted for l2.  ncols = 1 unless class_conditional. */
int sgmcmc_calibration_error(const double* keys, int64_t elem_stride, int64_t col_stride, const int32_t* perm,
                             const int64_t* target, int class_conditional, int n, int ncols, const double* bounds,
                             int num_bins, int l2, double* col_err, double* out, void* stream);
/* sklearn.metrics.roc_auc_score / average_precision_score as exp_utils.py:368-373 calls them: rows [0, n_pos) of
 * scores are the positives (in-distribution), [n_pos, n) the negatives; perm = sgmcmc_stable_order of scores.
 * Integer cumulative TP / FP at each distinct threshold from the top; out[0] = 2 area / (2.0 P Nn) with
 * 2 area = sum dFP (TP_prev + TP) in integers, out[1] = sum (R_k - R_{k-1}) P_k over the thresholds in descending
 * order, out[2] = 1 if a score is NaN (out[0], out[1] NaN then), else 0.  0 < n_pos < n. */
int sgmcmc_rank_metrics(const double* scores, const int32_t* perm, int n, int n_pos, double* out, void* stream);

/* ---- Uncertainty of a posterior ensemble: entropy decomposition, proper scores, risk-coverage (fp64, deterministic) ---
 * The reference has no such function; this is the definition.
 *
 * sgmcmc_uncertainty_rows: one pass over acc [samples][rows][classes] = [E][N][C], per-sample NORMALISED
 * log-probabilities (the table of sgmcmc_ensemble_probs, same precondition: the kernel does not renormalise, so a table
 * whose rows do not sum to 1 under exp gives the formulas below applied to it as it stands).  Per row n:
 *  1. probs[n, :], max_prob[n], pred[n], hit[n]: pbar = softmax(logsumexp_e acc[e, n, :] - log E), its maximum, the first
 *     index of the maximum and pred == labels -- the very instruction sequence of sgmcmc_ensemble_probs: the same bits.
 *  2. margin[n] = max_prob - (the largest pbar_c over c != pred): 0 when the maximum occurs twice; for C = 1 the second
 *     largest is 0.
 *  3. entropy[n] = -sum_c pbar_c log pbar_c, a term with pbar_c = 0 being 0 (nats).
 *  4. expected_entropy[n] = -(sum_c h_c) / E with h_c = sum_e p log p, p = exp(acc[e, n, c]), the term of acc = -inf
 *     being 0: the mean over the samples of each sample's own entropy.  h_c is formed as exp(m_c) sum_e x exp(x - m_c),
 *     x = acc[e, n, c], on the running maximum m_c of 1.'s log-sum-exp and from its exponentials (rescaled by the same
 *     factor whenever the maximum moves), so an entry costs one exp.  The samples are added in order of e; the sums
 *     over the classes of 3. and 4. run in order of c with Neumaier's compensation (sum and carried error, added at
 *     the end), which keeps a 128-term sum within an ulp or two of its exact value.
 *  5. mutual_info[n] = entropy - expected_entropy, and 0 where that difference is negative (Jensen: it is not in exact
 *     arithmetic; the clamp removes rounding of the order C eps).
 *  6. disagreement[n] = #{e : first argmax_c acc[e, n, :] != pred[n]} / E, the count an integer.
 *  7. with labels, y = labels[n]: nll[n] = -log pbar_y (+inf where pbar_y = 0); brier[n] = sum_c (pbar_c - [c == y])^2,
 *     c ascending.  A label outside 0 .. C-1 names a class of probability 0: nll = +inf, brier = sum_c pbar_c^2.
 * NaN rule: a NaN anywhere in the E x C entries of a row makes every probability of that row NaN, hence every
 * floating-point output of the row (disagreement included); pred = 0 then (sgmcmc_row_max's rule: the first NaN wins)
 * and hit = (labels[n] == 0).  Other rows are not touched.
 * labels, hit, nll, brier: all four NULL or all four given.  Limits: 1 <= classes <= SGMCMC_CALIB_MAX_CLASSES,
 * 1 <= samples, rows < 2^31; anything else, or a NULL pointer, returns hipErrorInvalidValue and launches nothing.
 * One launch; the table is read once (8 E N C bytes); every output entry is written. */
int sgmcmc_uncertainty_rows(const double* acc, const int64_t* labels, int samples, int rows, int classes, double* probs,
                            double* max_prob, int64_t* pred, int64_t* hit, double* margin, double* entropy,
                            double* expected_entropy, double* mutual_info, double* disagreement, double* nll,
                            double* brier, void* stream);
/* Risk-coverage curve of selective prediction.  scores [n]: higher = more confident; losses [n]: any fp64 values (1 - hit,
 * nll, ...); perm = sgmcmc_stable_order of scores (one column).  Rank k = 1 .. n counts the rows from the most confident
 * down.  Rows of equal score (-0.0 == 0.0) form a tie group of ranks (a, b]; with P(i) the sum of the losses of the first
 * i ranks,
 *     cum(k) = P(a) + (k - a) (P(b) - P(a)) / (b - a)   for a < k <= b,     risk[k - 1] = cum(k) / k,
 * the expectation of the selective risk at coverage k / n over a uniformly random order inside every tie group, so the
 * curve does not depend on the order of the rows.  It is evaluated as one division,
 * ((b - a) P(a) + (k - a) (P(b) - P(a))) / ((b - a) k): for integer-valued losses numerator and denominator are exact,
 * risk[k - 1] is the correctly rounded rational, and a permutation of the rows changes no bit.  P(b) == P(a) counts as a
 * group sum of 0 (also where both are +inf, so that an infinite loss gives +inf from its rank on).
 * out[0] = aurc = (sum_k risk[k - 1]) / n, out[1] = P(n) / n, the mean loss, out[2] = 1 if a score or a loss is NaN (then
 * out[0], out[1] and every risk entry are NaN), else 0.
 * Sums: the ranks are cut into 1024 consecutive chunks of ceil(n / 1024); P(i) = (the inclusive Hillis-Steele scan of the
 * chunk totals, at the chunk before i's) + (the losses of i's chunk before i, in rank order); aurc adds each chunk's
 * entries in rank order and then the 1024 chunk sums in order.  n <= SGMCMC_CALIB_MAX_ROWS.  One launch, one workgroup. */
int sgmcmc_risk_coverage(const double* scores, const double* losses, const int32_t* perm, int n, double* risk,
                         double* out, void* stream);

/* ---- Predictive scores of a regression posterior: CRPS, PIT, log density, variance split, quantiles (fp64, --------
 * deterministic).  The reference has no such function; this is the definition.
 *
 * mean [samples][rows][outputs] = [E][N][D], contiguous: the samples' predictive means.  scale: their standard
 * deviations, element (e, n, d) at scale[e * scale_se + n * scale_sn + d * scale_sd]; any stride may be 0, so that a
 * noise level per sample ([E]), per sample and output ([E, D]) or per entry ([E, N, D]) is read where it lies.  Per entry
 * (n, d) the posterior predictive is the equal-weight mixture of Normal(mu_e, sigma_e), with the CDF
 *     F(x) = (1/E) sum_e Phi((x - mu_e) / sigma_e),   Phi(z) = erfc(-z / sqrt 2) / 2   (both tails keep their accuracy).
 *
 * sgmcmc_gmix_rows, per entry:
 *  1. pred_mean = mbar = (sum_e mu_e) / E.
 *  2. var_aleatoric = (sum_e sigma_e^2) / E; var_epistemic = (sum_e (mu_e - mbar)^2) / E, in a second pass over the
 *     samples; var_total = var_aleatoric + var_epistemic, the mixture's variance.
 *  with y [N][D] (y, sq_err, lpd, pit, crps: all five NULL or all five given):
 *  3. sq_err = (y - mbar)^2.
 *  4. lpd = log (1/E) sum_e N(y; mu_e, sigma_e), the log-sum-exp of -z_e^2 / 2 - log sigma_e - log(2 pi) / 2 with
 *     z_e = (y - mu_e) / sigma_e, minus log E.
 *  5. pit = F(y).
 *  6. crps = (1/E) sum_i A(y - mu_i, sigma_i) - (1/E^2) [ sum_{i<j} A(mu_i - mu_j, sqrt(sigma_i^2 + sigma_j^2))
 *            + sum_i sigma_i / sqrt(pi) ],   A(m, s) = m erf(m / (s sqrt 2)) + 2 s phi(m / s) = E|Normal(m, s)|:
 *     the closed form of  integral (F(x) - 1[x >= y])^2 dx  for a Gaussian mixture (Grimit et al. 2006).
 * Sums.  The samples are dealt to 16 slices (e mod 16); a slice adds its terms in order of e with Neumaier's
 * compensation and the 16 slice sums are added in slice order, compensated again; the log-sum-exp runs per slice
 * and the slices are merged on their common maximum in slice order.  The pair sum of 6. cuts the samples into tiles of
 * SGMCMC_GMIX_TILE and an entry's triangle of tile pairs (I <= J, row by row) into S consecutive chunks, one workgroup
 * each, S = min(ceil(2048 / (N D)), ceil(P / 2)) with P the number of tile pairs: a function of (E, N, D) alone.  A thread
 * owns one i of tile I and every second j of tile J, adds its terms in order with compensation, the workgroup's 256
 * sums are added in an error-free (two-sum) tree, and the S partials of an entry are added in order as above.  Two
 * calls give the same bits.
 * NaN rule: a NaN among an entry's mu_e or its y, or a sigma_e that is not > 0, makes every floating-point output of that
 * entry NaN; other entries are not touched.
 * workspace: sgmcmc_gmix_workspace_bytes(samples, rows, outputs) bytes (-1 for sizes outside the limits), needed with
 * y only.  Limits: 1 <= samples <= SGMCMC_GMIX_MAX_SAMPLES, 1 <= rows, outputs, rows * outputs <= 2^30; anything
 * else, a negative stride or a missing pointer returns hipErrorInvalidValue and launches nothing.  Two launches with
 * y (E^2 / 2 erf + exp per entry), one without; nothing synchronises with the host. */
#define SGMCMC_GMIX_TILE 128
#define SGMCMC_GMIX_MAX_SAMPLES 32768
#define SGMCMC_GMIX_MAX_QUANTILES 64
#define SGMCMC_PIT_MAX_LEVELS 1024
int64_t sgmcmc_gmix_workspace_bytes(int samples, int rows, int outputs);
int sgmcmc_gmix_rows(const double* mean, const double* scale, int64_t scale_se, int64_t scale_sn, int64_t scale_sd,
                     const double* y, int samples, int rows, int outputs, void* workspace, int64_t workspace_bytes,
                     double* pred_mean, double* var_aleatoric, double* var_epistemic, double* var_total, double* sq_err,
                     double* lpd, double* pit, double* crps, void* stream);
/* Quantiles of the same mixtures: out[j][n][d] = q with F(q) = probs[j], j < n_probs <= SGMCMC_GMIX_MAX_QUANTILES, probs
 * and z = Phi^-1(probs) in DEVICE memory (fp64; the caller supplies z).  The root lies in the hull of the components' own
 * quantiles, lo = min_e (mu_e + sigma_e z) and hi = max_e (mu_e + sigma_e z): F(lo) <= p <= F(hi).  An end whose F already
 * meets p (lo == hi, as for E = 1; F(lo) >= p; F(hi) <= p) is returned as it stands -- E = 1 gives mu + sigma z.  Else the
 * bracket is refined by the secant through its ends (Illinois: the weight of an end kept twice is halved), by its
 * midpoint whenever the step before did not halve it or the secant point is not inside, until the ends are adjacent
 * doubles or F(x) == p, and for at most 256 steps; the end with the smaller |F - p| is returned (the lower on a tie).
 * Every F is the slice-wise sum of sgmcmc_gmix_rows' 5.  The NaN rule and the limits are sgmcmc_gmix_rows'. */
int sgmcmc_gmix_quantiles(const double* mean, const double* scale, int64_t scale_se, int64_t scale_sn, int64_t scale_sd,
                          int samples, int rows, int outputs, const double* probs, const double* z, int n_probs,
                          double* out, void* stream);
/* Calibration of PIT values u (one column per output; column c's value i at pit[c * col_stride + i * elem_stride], perm =
 * sgmcmc_stable_order of the columns), one workgroup per column.  With u_(1) <= ... <= u_(n) and W = 3 + n_levels +
 * n_central, out[c * W + ...]:
 *  [0] the Kolmogorov-Smirnov distance to the uniform, max_k max(k / n - u_(k), u_(k) - (k - 1) / n);
 *  [1] the calibration error of Kuleshov et al. 2018, (1 / n_levels) sum_j (count_j / n - levels[j])^2, the terms added
 *      in a fixed binary tree;
 *  [2] 1 if the column holds a NaN (then every other entry of the column's out is NaN), else 0;
 *  [3 + j] count_j = #{u <= levels[j]}, an integer;
 *  [3 + n_levels + i] #{(1 - c_i) / 2 <= u <= (1 + c_i) / 2} for c_i = central[i], an integer.
 * levels, central: DEVICE memory.  1 <= n <= SGMCMC_CALIB_MAX_ROWS, 1 <= n_levels <= SGMCMC_PIT_MAX_LEVELS,
 * 0 <= n_central <= SGMCMC_PIT_MAX_LEVELS, ncols <= 65535.  One launch. */
int sgmcmc_pit_calibration(const double* pit, int64_t elem_stride, int64_t col_stride, const int32_t* perm, int n,
                           int ncols, const double* levels, int n_levels, const double* central, int n_central,
                           double* out, void* stream);

/* ---- Between-chain diagnostics of stored draws: split-R-hat and effective sample size (fp64, deterministic) ----------
 * The reference has no such function; this is the definition (Gelman et al., BDA3 section 11.4-11.5; Geyer 1992;
 * Vehtari et al. 2021 without the rank normalisation).  x[m][s][q]: `chains` x `draws` x `quantities` values, fp32
 * (is_f64 = 0) or fp64, element (m, s, q) at x[m * chain_stride + s * draw_stride + q]; fp32 is widened on load and all
 * arithmetic is fp64.
 *  1. split != 0: n = draws / 2, every chain gives the sequences of its draws [0, n) and [draws - n, draws) (an odd
 *     count loses its middle draw, which is never read), J = 2 chains; split == 0: n = draws, J = chains.
 *  2. per sequence j and quantity: the mean mu_j, c_s = x_s - mu_j (two passes) and the biased autocovariance
 *     a_j[t] = (1/n) sum_{s=0}^{n-1-t} c_s c_{s+t}, t = 0 .. n-1.
 *  3. W = mean_j a_j[0] n/(n-1); B/n = var_j(mu_j) with ddof = 1 (0 if J = 1); var+ = W (n-1)/n + B/n.
 *  4. rhat = sqrt(var+ / W).
 *  5. rho_0 = 1, rho_t = 1 - (W - mean_j a_j[t]) / var+ for t >= 1.
 *  6. P_k = rho_{2k} + rho_{2k+1}, k = 0 .. n/2 - 1; K = the smallest k >= 1 with P_k <= 0, or n/2 if there is none;
 *     P'_0 = P_0, P'_k = min(P'_{k-1}, P_k).
 *  7. tau = -1 + 2 sum_{k<K} P'_k, raised to at least 1 / log10(J n); ess = J n / tau.
 *  8. a quantity with a non-finite draw in one of its sequences, or with W = 0, gives NaN for rhat and ess (and
 *     pairs = 0); nothing else is special-cased.
 * Every sum runs in an order fixed by (chains, draws, split): the mean as SGMCMC_DIAG_MEAN_WAYS interleaved partial sums
 * added in order, a_j[t] over ascending s, sums over j in ascending j (the means by Welford's update).  A quantity's
 * result does not depend on the other quantities of the call, and sgmcmc_chain_rhat equals the rhat of sgmcmc_chain_ess
 * bit for bit.  Limits: 4 <= n <= SGMCMC_DIAG_MAX_SEQ, J <= SGMCMC_DIAG_MAX_CHAINS, strides >= 0; anything else returns
 * hipErrorInvalidValue and launches nothing. */
#define SGMCMC_DIAG_MAX_SEQ 512    /* n: a [n][SGMCMC_DIAG_TILE] fp64 tile of centred draws is staged in LDS (128 KiB) */
#define SGMCMC_DIAG_MAX_CHAINS 64  /* J */
#define SGMCMC_DIAG_LAG_BLOCK 32   /* lags per pass of sgmcmc_chain_ess over the sequences */
#define SGMCMC_DIAG_TILE 32        /* quantities per workgroup of sgmcmc_chain_ess */
#define SGMCMC_DIAG_MEAN_WAYS 8    /* partial sums of every mean */

/* rhat [quantities]: steps 1-4 and 8.  One launch, one thread per quantity, the data read twice. */
int sgmcmc_chain_rhat(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains, int draws,
                      int64_t quantities, int split, double* rhat, void* stream);
/* ess [quantities]: steps 1-8; rhat [quantities] (may be NULL); pairs [quantities] (int32, may be NULL) receives K.
 * One launch: a workgroup per SGMCMC_DIAG_TILE quantities walks the lags in blocks of SGMCMC_DIAG_LAG_BLOCK, re-reading
 * the sequences once per block, and stops after the block in which the last quantity of its tile found its K (lags
 * above 2K + 1 enter no result): one pass for well-mixed chains, n / SGMCMC_DIAG_LAG_BLOCK passes at worst. */
int sgmcmc_chain_ess(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains, int draws,
                     int64_t quantities, int split, double* ess, double* rhat, int32_t* pairs, void* stream);

/* ---- Rank-normalised R-hat, bulk ESS and tail ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) ---------------
 * The moment-based definition above assumes a finite mean and variance; under heavy-tailed priors (cauchy, student-t
 * with few degrees of freedom, horseshoe) it says little.  This is the definition of the rank-normalised one.  x, split,
 * n, J and the sequences are as above; N = J n.  For one quantity v_1 .. v_N are the draws that enter the sequences, in
 * sequence order (sequence 0 first; with split and an odd count a chain's middle draw enters nothing); fp32 is widened
 * on load; -0.0 counts as, and is written as, +0.0.  Rhat(.), Ess(.) and K(.) are steps 2-8 above applied to J
 * sequences of n values without a further split.
 *   average rank   r_i = #{j : v_j < v_i} + (#{j : v_j = v_i} + 1) / 2 over all N draws (the second count includes i):
 *                  integer counts, so ranks are exact
 *   normal score   z(v)_i = ndtri((r_i - 3/8) / (N + 1/4)): numerator and denominator are exact in fp64, the quotient is
 *                  one correctly rounded division; ndtri is the inverse of the standard normal distribution function
 *                  (Cephes' rational approximations)
 *   quantile       type 7 (numpy's "linear"): pos = (N - 1) p, lo = floor(pos), hi = min(lo + 1, N - 1),
 *                  q_p(v) = v_(lo) + (v_(hi) - v_(lo)) (pos - lo), v_(k) the k-th smallest counted from 0; every
 *                  operation is rounded once (nothing is contracted into an fma), and in numpy's order: with
 *                  d = v_(hi) - v_(lo) and t = pos - lo, v_(lo) + d t if t < 0.5, else v_(hi) - d (1 - t) -- the same
 *                  number, interpolated from the nearer neighbour, so that q_p equals np.quantile(method="linear")
 *                  bit for bit; the median is q_0.5
 *   results        rhat     = max(Rhat(z(v)), Rhat(z(|v - q_0.5(v)|)))        (the subtraction rounded once)
 *                  ess_bulk = Ess(z(v))
 *                  ess_tail = min(Ess(1[v <= q_plo(v)]), Ess(1[v <= q_phi(v)])), (plo, phi) = (0.05, 0.95) by default
 *   NaN rule       a quantity with a non-finite draw gives NaN in all three; otherwise rhat is NaN if either part is
 *                  (a constant column), ess_tail is NaN if either indicator's Ess is (a constant indicator: enough
 *                  draws tie at an extreme).
 * For even N the two middle draws have mathematically equal folded values, and whether they tie in floating point
 * decides two ranks: hence the singly rounded median and subtraction (frac = 0.5: the product is exact).
 * The three entries below produce the [J][n][Q] arrays; sgmcmc_chain_rhat / sgmcmc_chain_ess (chains = J, draws = n,
 * split = 0) turn them into the parts, and the caller combines the parts (bnn_priors_amd/diagnostics.py rank_rhat_ess).
 * No atomics; ranks are counted, so no schedule can change a bit; a quantity's result depends on its own column only.
 * The caller provides every buffer; nothing is allocated and nothing synchronises.  An argument set that
 * sgmcmc_chain_ess refuses, a NULL required pointer or a p outside (0, 1) returns hipErrorInvalidValue and launches
 * nothing. */
#define SGMCMC_RANK_OWN 16         /* draws of its quantity that a thread of the score kernel ranks */
#define SGMCMC_RANK_MAX_PROBS 3    /* quantile probabilities per call */

/* z [J][n][quantities] (fp64, contiguous): the normal scores of x, or with centre [quantities] != NULL of
 * |x - centre|.  nprobs > 0: probs [nprobs] (HOST memory, each in (0, 1), at most SGMCMC_RANK_MAX_PROBS) and ostat
 * [2 nprobs][quantities] receives the order statistics v_(lo), v_(hi) of probs[i] in rows 2 i, 2 i + 1 (of the folded
 * values if centre is given); nprobs = 0: probs and ostat may be NULL.  A quantity with a non-finite (folded) draw gets
 * NaN in all of z and ostat.  One launch: lane = quantity, a thread keeps SGMCMC_RANK_OWN draws in registers and
 * streams the N draws of its column, counting less and equal; N^2 quantities comparisons. */
int sgmcmc_chain_rank_scores(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains,
                             int draws, int64_t quantities, int split, const double* centre, const double* probs,
                             int nprobs, double* z, double* ostat, void* stream);
/* out [nprobs][quantities]: q_p of probs[i] (HOST memory) from ostat as sgmcmc_chain_rank_scores wrote it for the same
 * (chains, draws, split, probs). */
int sgmcmc_chain_quantiles(const double* ostat, int chains, int draws, int split, const double* probs, int nprobs,
                           int64_t quantities, double* out, void* stream);
/* lower, upper [J][n][quantities] (fp32, contiguous; 0 and 1 are exact): 1[x <= q_lower[q]] and 1[x <= q_upper[q]]. */
int sgmcmc_chain_tail_indicators(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains,
                                 int draws, int64_t quantities, int split, const double* q_lower,
                                 const double* q_upper, float* lower, float* upper, void* stream);

/* ---- Posterior summaries with Monte Carlo standard errors (fp64, deterministic) ---------------------------------------
 * What the posterior is and how precisely the stored draws pin it down: mean, sd, quantiles, the highest-density
 * interval, and the Monte Carlo standard error (MCSE) of the mean, the sd and every quantile.  The reference has no such
 * function; this is the definition (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; the R package posterior's
 * mcse_mean, mcse_sd, mcse_quantile; ArviZ's unimodal HDI), restated in tests/summary_reference.py.  x, split, n, J, the
 * sequences and N = J n are as in the rank-normalised section; v_1 .. v_N are the draws that enter the sequences, in
 * sequence order (draw i = j n + s; with split and an odd count a chain's middle draw enters nothing), v_(k) the k-th
 * smallest counted from 0; fp32 is widened on load and all arithmetic is fp64; every operation is rounded once (nothing
 * is contracted into an fma); -0.0 counts as, and is written as, +0.0.  Ess(.) is sgmcmc_chain_ess applied to J
 * sequences of n values (for v itself: to x with the call's split).
 *   sums           every sum over the draws runs over i = 0 .. N-1 as SGMCMC_DIAG_MEAN_WAYS interleaved partial sums
 *                  (i = r mod SGMCMC_DIAG_MEAN_WAYS, each in ascending i, from +0.0) added in ascending r: an order fixed
 *                  by (chains, draws, split)
 *   mean           sum_i v_i / N; a column whose draws are all equal has that value as its mean (the sum of N copies may
 *                  round away from it)
 *   moments        c_i = v_i - mean, m2 = sum_i c_i^2 / N, m4 = sum_i (c_i^2)^2 / N
 *   sd             sqrt(m2 N / (N - 1))
 *   ess_mean       Ess(v);   mcse_mean = sd / sqrt(ess_mean)
 *   ess_sd         Ess(c^2); mcse_sd = sqrt((m4 - m2 m2) / ess_sd / m2 / 4)   (posterior::mcse_sd, kurtosis-aware)
 *   quantile q_p   any p in (0, 1): the type-7 definition of the rank-normalised section in numpy's operation order,
 *                  read from the sorted column; bit-equal to sgmcmc_chain_quantiles
 *   mcse_quantile  ess_q(p) = Ess(1[v <= q_p]); alpha = ess_q p + 1, beta = ess_q (1 - p) + 1;
 *                  a = I^-1(0.1586553; alpha, beta), b = I^-1(0.8413447; alpha, beta), I^-1 the inverse of the
 *                  regularised incomplete beta function x -> I_x(alpha, beta);
 *                  lo = max(floor(a N), 1) - 1, hi = min(ceil(b N), N) - 1; mcse_q(p) = (v_(hi) - v_(lo)) / 2
 *   HDI of mass h  k = floor(h N) (1 <= k <= N - 1 is required), w_i = v_(i+k) - v_(i) for i = 0 .. N-k-1, i* the first
 *                  i that attains the minimum; the interval is (v_(i*), v_(i*+k))
 *   NaN rule       a quantity with a non-finite draw gives NaN in everything (lo = hi = -1).  A quantity with m2 = 0 (a
 *                  constant column) gives its mean and quantiles, sd = 0, HDI bounds equal to the value, and NaN for
 *                  every ess and mcse.  A constant indicator (W = 0 in its Ess) gives NaN for that ess_q and mcse_q
 *                  (a = b = NaN, lo = hi = -1).
 * a and b are the only results that are not fixed to the bit by this text: I^-1 is evaluated on the device by a bracketed
 * Newton search on I_x (a continued fraction; the beta function through the remainders of Stirling's formula, which
 * keeps a relative error of a few 10^-15 at alpha, beta of 10^4), and lo, hi and mcse_q inherit a difference only where
 * a N or b N lies within that error of an integer.
 * The caller provides every buffer; nothing is allocated, nothing synchronises, everything runs on the given stream; no
 * atomics; a quantity's result depends on its own column only, whatever the grid, the tile or the chunk.  Limits: those
 * of sgmcmc_chain_ess and N <= SGMCMC_SUMMARY_MAX_DRAWS; anything else, a NULL required pointer or a probability
 * outside (0, 1) returns hipErrorInvalidValue and launches nothing. */
#define SGMCMC_SUMMARY_MAX_DRAWS 16384 /* N: one fp64 column of the sort's LDS tile (128 KiB) */
#define SGMCMC_SUMMARY_MAX_TILE 64     /* quantities per workgroup of the sort, at most */

/* TQ, the quantities per workgroup of sgmcmc_summary_sort at N = total_draws: the most columns of N_pad fp64 (N_pad the
 * next power of two, at least 4) that fit 128 KiB, SGMCMC_SUMMARY_MAX_TILE at most; 0 for an N that is refused.  Host
 * arithmetic only. */
int sgmcmc_summary_tile_quantities(int total_draws);
/* sorted [N][quantities] (fp64, contiguous): every column's draws in ascending order, zeros as +0.0; a column with a
 * non-finite draw is NaN throughout.  One launch: a workgroup stages an [N_pad][TQ] tile in LDS, pads it with +inf
 * after deciding the non-finite rule, and sorts its columns with a bitonic network, O(N log^2 N) per column. */
int sgmcmc_summary_sort(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains, int draws,
                        int64_t quantities, int split, double* sorted, void* stream);
/* mean, sd, m2, m4 [quantities] and csq [J][n][quantities] (fp64, contiguous) = c^2, the input of ess_sd (NaN for a
 * quantity with a non-finite draw).  One launch, lane = quantity and one thread group per partial sum, the data read
 * twice. */
int sgmcmc_summary_moments(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains, int draws,
                           int64_t quantities, int split, double* mean, double* sd, double* m2, double* m4,
                           double* csq, void* stream);
/* out [quantities]: q_prob from `sorted` as sgmcmc_summary_sort wrote it for the same (chains, draws, split). */
int sgmcmc_summary_quantile(const double* sorted, int chains, int draws, int split, double prob, int64_t quantities,
                            double* out, void* stream);
/* lower, upper [quantities]: the HDI of `mass` from `sorted`. */
int sgmcmc_summary_hdi(const double* sorted, int chains, int draws, int split, double mass, int64_t quantities,
                       double* lower, double* upper, void* stream);
/* mcse_mean, mcse_sd [quantities] from sd, m2, m4 (sgmcmc_summary_moments), ess_mean = Ess(v) and ess_sd = Ess(c^2);
 * ess_mean is also WRITTEN: NaN where m2 = 0 (the per-sequence means inside Ess may leave a constant column a variance
 * at rounding level). */
int sgmcmc_summary_mcse(const double* sd, const double* m2, const double* m4, double* ess_mean, const double* ess_sd,
                        int64_t quantities, double* mcse_mean, double* mcse_sd, void* stream);
/* mcse [quantities]: mcse_q(prob) from `sorted` and ess_q [quantities] = Ess(1[v <= q_prob]); a, b [quantities] (fp64)
 * and lo, hi [quantities] (int32) receive the parts and may each be NULL. */
int sgmcmc_summary_mcse_quantile(const double* sorted, int chains, int draws, int split, double prob,
                                 const double* ess_q, int64_t quantities, double* mcse, double* a, double* b,
                                 int32_t* lo, int32_t* hi, void* stream);

/* ---- Model comparison: PSIS-LOO with Pareto-k and WAIC (fp64, deterministic) -------------------------------------------
 * Vehtari, Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024; Watanabe 2010; the generalised Pareto fit of
 * Zhang and Stephens 2009.  The reference has no such function (its only model-comparison number is the log-mean-exp of
 * exp_utils.evaluate_marglik); this is the definition, restated in tests/psis_reference.py.
 * ll[s][i]: `draws` (S) x `observations` (N) values of log p(y_i | theta_s), fp32 (is_f64 = 0) or fp64, element (s, i) at
 * table[s * draw_stride + i]; with is_ratio != 0 the table holds the log ratios r = -ll instead (the negation is exact).
 * fp32 is widened on load, all arithmetic is fp64, every operation is rounded once (nothing is contracted into an fma).
 * r_eff [N] (fp64, may be NULL: 1 everywhere) is the relative efficiency of the draws.
 * Per observation (column) i, with r = -ll:
 *  1. x_s = r_s - max_s r_s (one rounding).
 *  2. M = ceil(min(0.2 S, 3 sqrt(S / r_eff))), at most SGMCMC_PSIS_MAX_TAIL (which binds only for S > 2720 with
 *     r_eff < 1); cut = max(x_(S-M-1), log DBL_MIN) with x_(k) the k-th smallest counted from 0 and log DBL_MIN the
 *     constant SGMCMC_PSIS_LOG_DBL_MIN; ec = exp(cut).
 *  3. the tail: the draws with x_s > cut (strict, exact), n2 of them (n2 <= M), in ascending order, ties by draw index.
 *     n2 <= 4: khat = +inf, nothing is smoothed.
 *  4. else t_j = exp(x_tail_j) - ec, j = 0 .. n2-1; m = 30 + floor(sqrt(n2));
 *     b_j = 1 / t_(n2-1) + (1 - sqrt(m / (j - 1/2))) / (3 t_(floor(n2/4 + 1/2) - 1)), j = 1 .. m;
 *     kappa_j = (sum_i log1p(-b_j t_i)) / n2;  L_j = n2 (log(-b_j / kappa_j) - kappa_j - 1);
 *     w_j = 1 / sum_l exp(L_l - L_j);  bbar = sum_j b_j w_j;  kappa = (sum_i log1p(-bbar t_i)) / n2;
 *     sigma = -kappa / bbar;  khat = (n2 kappa + 5) / (n2 + 10).  Every sum runs over ascending index.
 *  5. khat finite: tail element j becomes log(sigma expm1(-khat log1p(-p_j)) / khat + ec), p_j = (j + 1/2) / n2
 *     (khat = 0: log(-sigma log1p(-p_j) + ec)).
 *  6. x_s <- min(x_s, 0); lw_s = x_s - logsumexp_s x, logsumexp_s v = max_s v + log sum_s exp(v_s - max_s v) over
 *     ascending s.
 * Pointwise outputs (rows of `pointwise` [SGMCMC_PSIS_POINTWISE][N], in this order):
 *     pareto_k = khat;  elpd_loo = logsumexp_s (lw_s + ll_s);  lppd = logsumexp_s ll_s - log S;
 *     p_loo = lppd - elpd_loo;  p_waic = sum_s (ll_s - mean_s ll)^2 / (S - 1) (two passes);  elpd_waic = lppd - p_waic.
 * NaN rule: a column with a non-finite ll, or whose r_eff is not a positive finite number, gives NaN in every output
 * (M = n2 = 0); nothing else is special-cased.  A constant column has an empty tail, khat = +inf, uniform weights.
 * Totals (`totals` [SGMCMC_PSIS_TOTALS], device memory): sum_i elpd_loo, se(elpd_loo), sum_i p_loo, sum_i lppd,
 * sum_i elpd_waic, se(elpd_waic), sum_i p_waic, #{khat > k_threshold}, max_i khat (NaN if one is NaN), with
 * se(v) = sqrt(N var_i(v, ddof = 1)) in two passes; every sum over i in an order fixed by N alone (256 interleaved
 * partial sums in ascending i, then a fixed tree).  The caller passes k_threshold = min(1 - 1 / log10(S), 0.7).
 * The caller provides every buffer; nothing is allocated, nothing synchronises, everything runs on the given stream;
 * no atomics; the tail is found by counting, so no schedule changes a bit; a column's result depends on that column
 * (and its r_eff) only, and the chunking changes no bit.  Limits: SGMCMC_PSIS_MIN_DRAWS <= S <= SGMCMC_PSIS_MAX_DRAWS
 * (counts fit int32, the tail's rows uint16), N >= 1, draw_stride >= N; anything else, a NULL required pointer or a
 * workspace too small for 64 observations (for N, if N < 64) returns hipErrorInvalidValue and launches nothing. */
#define SGMCMC_PSIS_MIN_DRAWS 5
#define SGMCMC_PSIS_MAX_DRAWS 32768
#define SGMCMC_PSIS_MAX_TAIL 544   /* ceil(3 sqrt(32768)) */
#define SGMCMC_PSIS_OWN 16         /* draws of its column that a thread of the selection kernel places */
#define SGMCMC_PSIS_POINTWISE 6
#define SGMCMC_PSIS_TOTALS 9
#define SGMCMC_PSIS_LOG_DBL_MIN (-708.3964185322641) /* the double nearest log(2^-1022) */

/* Bytes of workspace with which `observations` columns are one chunk: per observation 8 rows + 64 + 2 S, rows =
 * min(ceil(0.2 S), SGMCMC_PSIS_MAX_TAIL) with r_eff, else min(that, ceil(3 sqrt(S))).  -1 for a refused shape.
 * A chunk of W observations lies in the workspace as tail [rows][W] fp64 (row 0: the largest), record [6][W] fp64,
 * counters [4][W] int32 and pos [S][W] uint16 (a draw's tail row, 0xffff outside the tail), in this order. */
int64_t sgmcmc_psis_workspace_bytes(int draws, int64_t observations, int has_r_eff);
/* Steps 1-6 and the pointwise outputs.  workspace (8-byte aligned): all N observations at once if workspace_bytes
 * allows, else chunks of the largest multiple of 64 that fits.  Optional outputs (may be NULL): fit [2][N] fp64 (sigma,
 * NaN without a fit; cut), counts [2][N] int32 (M; n2), lw [S][N] fp64 (contiguous).  Per chunk four launches: one
 * thread per column streams the table (statistics, M), the selection kernel places the tail by counting (S^2 N
 * compares), one thread per column fits (m + 1 passes of log1p over its tail), one thread per column finishes. */
int sgmcmc_psis_loo(const void* table, int is_f64, int is_ratio, int64_t draw_stride, int draws, int64_t observations,
                    const double* r_eff, void* workspace, int64_t workspace_bytes, double* pointwise, double* fit,
                    int32_t* counts, double* lw, void* stream);
/* The totals of pointwise [SGMCMC_PSIS_POINTWISE][N] as sgmcmc_psis_loo wrote it.  One launch of one workgroup. */
int sgmcmc_psis_totals(const double* pointwise, int64_t observations, double k_threshold, double* totals,
                       void* stream);

/* ---- Power-scaling sensitivity: does the prior matter? (fp64, deterministic) -------------------------------------------
 * Kallioinen, Paananen, Buerkner, Vehtari 2023 (the R package priorsense).  The reference has no such function; this is
 * the definition -- it governs, not the R package -- restated in tests/powerscale_reference.py.  The prior, or the
 * likelihood, is raised to a power alpha near 1 by importance-reweighting the stored draws (log ratios
 * (alpha - 1) log p, smoothed by sgmcmc_psis_loo with is_ratio); what this section adds is how far every quantity's
 * weighted distribution moves.
 * x[m][s][q]: `chains` (M) x `draws` (S) x `quantities` (Q), fp32 (is_f64 = 0) or fp64, element (m, s, q) at
 * x[m * chain_stride + s * draw_stride + q], read in place.  Draw t = m S + s, N = M S; there is no splitting.  fp32 is
 * widened on load, all arithmetic is fp64, every operation is rounded once (nothing is contracted into an fma).
 * Keyed sort (sgmcmc_powerscale_sort): every column is sorted ascending by value, ties by ascending draw index t -- a
 * total order, so the result is unique.  sorted[i][q] (fp64) is the value and order[i][q] (uint16) the draw index at rank
 * i.  -0.0 counts as, and is written as, +0.0.  A column with a non-finite draw is NaN throughout `sorted`; its `order`
 * is unspecified (but below N).
 * Weighted distance and moments (sgmcmc_powerscale_distance): w[t][a], `vectors` (A) weight vectors, fp64, linear (not
 * log) and non-negative, element (t, a) at weights[t * A + a].  For vector a and quantity q, v_i = sorted[i][q] and
 * w_i = w[order[i][q]][a]:
 *   W        sum_t w[t][a] over ascending t from +0.0, one accumulator (a function of a only)
 *   C_i      sum_{k <= i} w_k over ascending i from +0.0;  for i = 0 .. N-2:
 *            Q_i = C_i / W,  P_i = (double)(i + 1) / N,  d_i = v_(i+1) - v_i,  s_i = P_i + Q_i,
 *            delta_i = (Q_i - P_i) / s_i
 *   g(delta) (1 - delta) log1p(-delta) + (1 + delta) log1p(delta) with 0 (-inf) = 0, so g(+-1) = 2 ln 2:
 *            |delta| < 1/4: the series sum_{k=1..16} delta^2k / (k (2k - 1)) by Horner in x = delta delta,
 *            acc = 0; for k = 16 .. 1: acc = (acc + c_k) x, c_k the double nearest 1 / (k (2k - 1));
 *            otherwise t1 = (1 - delta) log1p(-delta) (0 for delta >= 1), t2 = (1 + delta) log1p(delta) (0 for
 *            delta <= -1), g = t1 + t2.  (The plain form P log2(P / M) + Q log2(Q / M) cancels at alpha near 1 and is
 *            not used.)
 *   den      sum_i d_i s_i;  num = (sum_i (d_i s_i) g(delta_i)) / SGMCMC_POWERSCALE_TWO_LN2;  dist = sqrt(num / den):
 *            the normalised cumulative Jensen-Shannon distance between the unweighted and the weighted ECDF, in [0, 1]
 *   wmean    (sum_i w_i v_i) / W over i = 0 .. N-1;  wsd = sqrt((sum_i w_i ((v_i - wmean) (v_i - wmean))) / W)
 * Every term is non-negative; every sum runs over ascending i from +0.0 with one accumulator.  dist, wmean and wsd are
 * [A][Q] fp64, element (a, q) at out[a * out_stride + q].
 * Rules: a column with a non-finite draw gives NaN in all three.  A weight vector with a non-finite or negative entry, or
 * whose W is not a positive finite number, gives NaN for all its quantities.  A column whose draws are all equal gives
 * dist = 0 (den = 0), wmean = that value and wsd = 0.  A zero weight is legal.
 * log1p is the only operation not fixed to the bit by this text, and it enters only where |delta| >= 1/4.
 * The caller provides every buffer (sorted and order of a chunk of quantities: 10 bytes per draw and quantity); nothing
 * is allocated, nothing synchronises, everything runs on the given stream; no atomics; a quantity's result depends on
 * its own column and its weight vector only, whatever the grid, the tile or the chunk.  Limits:
 * SGMCMC_PSIS_MIN_DRAWS <= N <= SGMCMC_POWERSCALE_MAX_DRAWS, 1 <= A <= 65535, out_stride >= Q; anything else or a NULL
 * pointer returns hipErrorInvalidValue and launches nothing. */
#define SGMCMC_POWERSCALE_MAX_DRAWS 8192  /* N: one column of the sort's LDS tile; the weight vector is 64 KiB of LDS */
#define SGMCMC_POWERSCALE_TILE_CELLS 8192 /* cells of the sort's tile, an fp64 value and a uint16 index each: 80 KiB */
#define SGMCMC_POWERSCALE_TWO_LN2 1.3862943611198906 /* the double nearest 2 ln 2 */

/* TQ, the quantities per workgroup of sgmcmc_powerscale_sort at N = total_draws:
 * min(64, SGMCMC_POWERSCALE_TILE_CELLS / N_pad), N_pad the next power of two (at least 8); 0 for an N that is refused.
 * Host arithmetic only. */
int sgmcmc_powerscale_tile_quantities(int total_draws);
/* sorted [N][quantities] (fp64) and order [N][quantities] (uint16), both contiguous.  One launch: a workgroup stages an
 * [N_pad][TQ] tile of values and draw indices in LDS, pads it with (+inf, own row) after deciding the non-finite rule, and
 * sorts its columns with the bitonic network of sgmcmc_summary_sort, the indices travelling with their values. */
int sgmcmc_powerscale_sort(const void* x, int is_f64, int64_t chain_stride, int64_t draw_stride, int chains, int draws,
                           int64_t quantities, double* sorted, uint16_t* order, void* stream);
/* dist, wmean, wsd from `sorted` and `order` as sgmcmc_powerscale_sort wrote them for N = total_draws.  One launch, lane
 * = quantity, one grid row per weight vector, the vector staged in LDS. */
int sgmcmc_powerscale_distance(const double* sorted, const uint16_t* order, int total_draws, int64_t quantities,
                               const double* weights, int vectors, int64_t out_stride, double* dist, double* wmean,
                               double* wsd, void* stream);

/* ---- Model averaging: stacking, pseudo-BMA and pseudo-BMA+ weights (fp64, deterministic) ------------------------------
 * Yao, Vehtari, Simpson, Gelman 2018.  The reference has no such function; this is the definition, restated in
 * tests/weights_reference.py.  P[k][i]: `models` (K) x `observations` (N) pointwise elpd values (sgmcmc_psis_loo's
 * elpd_loo row of each model, or any other pointwise log density), fp64, element (k, i) at P[k * model_stride + i], read
 * in place.  All arithmetic is fp64 and every operation is rounded once (nothing is contracted into an fma).
 * Sums over i: the observations are cut into slices of SGMCMC_WEIGHTS_SLICE = 1,024; a slice's sum is 256 partial sums
 * and the fixed tree (partial t += partial t + 128, then t + 64, ..., t + 1); the slices are added in ascending order.
 * Partial t of a slice holds, added in ascending order, elements t, t + 256, t + 512, t + 768 of the slice (stacking,
 * mixture, pseudo-BMA) or elements 4t .. 4t + 3 (the bootstrap, whose thread owns one Philox counter = four
 * observations).  Elements past N count as 0.  Sums over k and over slices start from 0 and ascend.  No atomics.
 *  1. Pseudo-BMA: elpd_k = sum_i P[k][i];  w_k = exp(elpd_k - max_j elpd_j) / sum_j exp(elpd_j - max_j elpd_j).
 *  2. Pseudo-BMA+ (Bayesian bootstrap), replicate b = 0 .. B-1: g_{b,i} = -log(u_{b,i}) in fp64, where u_{b,i} is the
 *     uniform (2 (x >> 9) + 1) 2^-24 (never 0) of word i & 3 of Philox4x32-10 with the 64-bit seed as key and the counter
 *     (quad_lo, quad_hi, b_lo, purpose << 28 | (stream & 0xfff) << 16 | b_hi16), quad = i >> 2, purpose =
 *     SGMCMC_WEIGHTS_NOISE_PURPOSE.  z_{b,k} = (N * sum_i g_{b,i} P[k][i]) / sum_i g_{b,i};  w_{b,.} = softmax_k z_{b,.}
 *     as in 1.  weights_k = (sum_b w_{b,k}) / B;  se_k = sqrt(sum_b (z_{b,k} - mean_b z_{.,k})^2 / (B - 1)), two passes
 *     (NaN for B = 1); the sums over b are 256 interleaved partial sums in ascending b, then the same tree.  Row b
 *     depends on (seed, stream, b) only: not on B, not on the workspace, not on the grid.
 *  3. Stacking: maximise f(w) = (1/N) sum_i log sum_k w_k exp(P[k][i]) over the simplex by the EM update of mixture
 *     proportions, from w = 1/K.  m_i = max_k P[k][i];  q_{k,i} = exp(P[k][i] - m_i);  one iteration is
 *         mix_i = sum_k w_k q_{k,i};  r_k = (sum_i q_{k,i} / mix_i) / N;  gap = max_k r_k - 1;
 *         lpd = sum_i (m_i + log mix_i);  then w_k <- w_k r_k.
 *     Because f is concave and sum_k w_k r_k = 1, f(w*) - f(w) <= gap at every iterate: gap is a certificate.  The
 *     iteration stops at the first iterate with gap <= tol, before its update is applied (converged), or when max_iter
 *     updates have been applied; r, gap and lpd are those of the returned w.  K = 1: w = 1, gap = 0, no update.
 *  4. Mixture log density for a given w: pointwise_i = m_i + log sum_k w_k q_{k,i};  total = sum_i pointwise_i.
 * NaN rule: a non-finite entry anywhere in P makes every output of 1-3 NaN (every weight depends on every observation)
 * and ends the stacking iteration (not converged); in 4 it makes that observation's pointwise value and the total NaN.
 * Nothing else is special-cased.
 * State record of a stacking run, `state` [SGMCMC_WEIGHTS_STATE] fp64 in device memory: updates applied, converged
 * (0 / 1), frozen (0 / 1), gap, lpd, tol, max_iter, reserved, w [32], r [32].
 * The caller provides every buffer; nothing is allocated, nothing synchronises, everything runs on the given stream.
 * Limits: 1 <= K <= SGMCMC_WEIGHTS_MAX_MODELS, N >= 1, model_stride >= N; anything else, a NULL pointer, a workspace
 * that is not 8-byte aligned or too small returns hipErrorInvalidValue and launches nothing. */
#define SGMCMC_WEIGHTS_SLICE 1024
#define SGMCMC_WEIGHTS_MAX_MODELS 32
#define SGMCMC_WEIGHTS_STATE 72
#define SGMCMC_WEIGHTS_NOISE_PURPOSE 4u /* 0-2 the sampler's, 3 augmentation's: the bootstrap shares words with none */

/* Bytes of workspace: the larger of 8 slices (K + 1) (+ 8 (K + 1) N with cache_q: m and q formed once) for stacking,
 * mixture and pseudo-BMA, and replicates * 8 slices (K + 1) for that many bootstrap replicates in one launch;
 * slices = ceil(N / 1024).  -1 for a refused shape or a size beyond int64. */
int64_t sgmcmc_weights_workspace_bytes(int models, int64_t observations, int64_t replicates, int cache_q);
/* Writes the state record (w = 1/K, tol >= 0, 0 <= max_iter <= 2^52) and, with cache_q != 0, m [N] and q [K][N] into the
 * workspace behind the partial sums.  One launch. */
int sgmcmc_stacking_init(const double* P, int64_t model_stride, int models, int64_t observations, double tol,
                         int64_t max_iter, int cache_q, void* workspace, int64_t workspace_bytes, double* state,
                         void* stream);
/* Enqueues `iters` iterations, two launches each: one workgroup per slice writes part [slices][K + 1] (sum q / mix per
 * model, sum (m + log mix)); one workgroup adds the slices, writes r, gap, lpd and applies the update.  A frozen state
 * (converged, max_iter reached, non-finite input) turns both into no-ops, so the result does not depend on how the
 * iterations are batched; max_iter + 1 iterations always freeze it.  Same P, workspace and cache_q as the init call. */
int sgmcmc_stacking_iterate(const double* P, int64_t model_stride, int models, int64_t observations, int cache_q,
                            int iters, void* workspace, int64_t workspace_bytes, double* state, void* stream);
/* Definition 4: w [K] in device memory -> pointwise [N] and total [1].  Two launches. */
int sgmcmc_mixture_lpd(const double* P, int64_t model_stride, int models, int64_t observations, const double* w,
                       void* workspace, int64_t workspace_bytes, double* pointwise, double* total, void* stream);
/* Definition 1: out [2][K] = the weights, then elpd_k.  Two launches. */
int sgmcmc_pseudo_bma(const double* P, int64_t model_stride, int models, int64_t observations, void* workspace,
                      int64_t workspace_bytes, double* out, void* stream);
/* Definition 2: z, w [B][K] (every row is written) and out [2][K] = weights, then se.  The replicates are walked in
 * chunks of as many as the workspace holds (at least one, at most 65,535): per chunk one launch of slices x chunk
 * workgroups and one of a thread per replicate; then one workgroup for the means and variances. */
int sgmcmc_bb_pseudo_bma(const double* P, int64_t model_stride, int models, int64_t observations, int64_t replicates,
                         uint64_t seed, uint32_t noise_stream, void* workspace, int64_t workspace_bytes, double* z,
                         double* w, double* out, void* stream);

/* ---- Fitting the data-driven priors to stacks of weight samples (fp64, deterministic) ----------------------------------
 * The reference fits its priors offline (scipy); this is the definition, restated in tests/prior_fit_reference.py.
 * A stack w [S, *shape] (fp32 or fp64) is read in place through a GEOMETRY: `events` events, numbered row-major over up
 * to four event dimensions (size, stride in elements; unused ones are size 1), each of F vectors (vector f at
 * f * f_stride) of P positions (position a at pos[a]).  Vector v = event * F + f; n = events * F vectors.  f_major != 0
 * tells the loader that f_stride exceeds the innermost event stride, so that a tile is walked f-first (coalesced along
 * the stack's fastest dimension); it changes no result.  All arithmetic is fp64, every operation rounded once.
 * Summation order: the events are cut into tiles of TE = max(1, min(SGMCMC_FIT_TILE_DOUBLES / (F (P | 1)),
 * SGMCMC_FIT_TILE_ROWS / F)) events; workgroup b of sgmcmc_fit_blocks() takes tiles b, b + blocks, ...  An accumulated
 * entry (of NE per pass) is cut into G = max(1, 256 / NE) slices; slice q adds rows (or events) q, q + G, ... of a tile
 * from 0 in ascending order, the tiles' sums are added in ascending order (compensated, Neumaier), the slices from 0 in
 * ascending order; of the workgroups' partials, slice q adds workgroups q, q + G, ... (compensated), and the slices are
 * added from 0 in ascending order.  Counts are integers.  No atomics.
 *  1. Moments.  Shift c_a = the median of position a of vectors 0, n / 2, n - 1 (0 if not finite); d = x - c.  From
 *     sum d_a, sum d_a d_b, sum d_a^3, sum d_a^4:  m = sum d / n;  mean = c + m;  cov_ab = (sum d_a d_b - sum d_a
 *     (sum d_b / n)) / (n - ddof);  with s_k = sum d^k / n:  m2 = s2 - m^2;  m3 = s3 - 3 m s2 + 2 m^3;
 *     m4 = s4 - 4 m s3 + 6 m^2 s2 - 3 m^4;  skew = m3 / m2^1.5;  kurt = m4 / m2^2 - 3 (population definitions; NaN for a
 *     column with m2 <= 0, whose var is reported as 0).  Pooled over the n P elements with delta_a = mean_a - mean of
 *     the means:  M2 = mean_a (m2 + delta^2), M3 = mean_a (m3 + 3 delta m2 + delta^3), M4 = mean_a (m4 + 4 delta m3
 *     + 6 delta^2 m2 + delta^4).  out: mean [P], cov [P][P], skew [P], kurt [P], var [P] (= m2), pooled {mean, var, skew,
 *     kurt}.  A non-finite element anywhere makes every output NaN; bad[0] counts them.
 *  2. Multivariate t by EM, in the standard parametrisation (mu, S, nu): an event's F vectors share one mixing variable,
 *     its scatter is I_F (x) S, D = F P.  State record, SGMCMC_FIT_STATE doubles: phase (0 iterating, 1 the pass at the
 *     returned parameters is due, 2 finished), iterations, converged, nu, sum_a log L_aa, loglik, df_at_bound, the last
 *     relative change, mu [25], L^-1 [25 x 25] and S [25 x 25] (row-major with row stride P; S = L L^T).  One iteration:
 *       A (one pass):  M_i = sum_f |L^-1 (x_if - mu)|^2;  u_i = (nu + D) / (nu + M_i);  sum u_i;  A = sum u_i sum_f d_if;
 *                      B = sum u_i sum_f d_if d_if^T;  sum (log u_i - u_i);  sum log1p(M_i / nu)
 *       B (one workgroup):  trace[iterations] = loglik(mu, S, nu) = events (lgamma((nu + D) / 2) - lgamma(nu / 2)
 *                      - D / 2 log(pi nu) - F sum log L_aa) - (nu + D) / 2 sum log1p(M_i / nu);  W = F sum u_i;
 *                      mu' = mu + A / W;  S' = (B - A (A / W)^T) / W (parameter-expanded: Kent, Tyler & Vardi 1994);
 *                      nu' = the root in [df_lo, df_hi] of log(nu'/2) - psi(nu'/2) + 1 + mean (log u_i - u_i)
 *                      + psi((nu + D) / 2) - log((nu + D) / 2) (Liu & Rubin 1995), by Newton steps kept inside a
 *                      bisection bracket until they move by less than 1e-15 nu' (the nearer bound if there is no root);
 *                      delta = max(|nu' - nu| / nu', |mu' - mu|_a / sqrt(S'_aa), |S' - S|_ab / sqrt(S'_aa S'_bb)).
 *     delta <= tol sets converged; then, or after max_iter iterations, one more pair A, B writes loglik at the returned
 *     parameters and finishes.  A finished state turns A and B into no-ops, so the result does not depend on how the
 *     iterations are batched.  A non-finite element, a non-finite log-likelihood or an S that is not positive definite
 *     finishes the fit with NaN parameters (not converged).  lgamma, psi and psi' are the recurrence up to x >= 10 and
 *     the asymptotic (Stirling) series through B_14.
 *  3. Element-wise sums at a given loc and beta over a P = F = 1 geometry, d = |x - loc|: out = {sum d, sum log d,
 *     sum d^beta, sum d^beta log d, sum d^beta log^2 d} over the elements with d > 0, d^beta = exp(beta log d);
 *     zeros[0] = #{d == 0}.  Thread t of workgroup b adds elements b 256 + t, + blocks 256, ... (compensated), the
 *     workgroup the fixed tree (t += t + 128, ..., t + 1).
 * The caller provides every buffer (part: (blocks + 1) * SGMCMC_FIT_PART doubles, counts: blocks int64); nothing is
 * allocated, nothing synchronises.  Limits: 1 <= P <= SGMCMC_FILTER_MAX_P, 1 <= F <= SGMCMC_FIT_TILE_ROWS,
 * F (P | 1) <= SGMCMC_FIT_TILE_DOUBLES, events F < 2^31, strides and offsets >= 0, the product of the sizes = events;
 * anything else or a NULL pointer returns hipErrorInvalidValue and launches nothing. */
#define SGMCMC_FIT_TILE_DOUBLES 5120
#define SGMCMC_FIT_TILE_ROWS 512
#define SGMCMC_FIT_MAX_BLOCKS 1024
#define SGMCMC_FIT_PART 408
#define SGMCMC_FIT_STATE 1288
typedef struct sgmcmc_fit_geometry {
  int32_t P, F, f_major, reserved;
  int64_t events;
  int64_t size[4], stride[4];
  int64_t f_stride;
  int64_t pos[SGMCMC_FILTER_MAX_P];
} sgmcmc_fit_geometry;

/* Workgroups of a pass (= partial records), a function of the sizes alone; -1 for a refused shape. */
int sgmcmc_fit_blocks(int P, int F, int64_t events);
/* Definition 1: one pass and one workgroup that adds its partials.  out [P P + 4 P + 4], bad [1]. */
int sgmcmc_fit_moments(const void* w, int dtype, const sgmcmc_fit_geometry* geometry, int ddof, double* part,
                       int64_t* counts, double* out, int64_t* bad, void* stream);
/* Writes the state record of definition 2: mu = mean [P], S = cov [P][P] (df - 2) / df, nu = df > 2.  One launch. */
int sgmcmc_fit_mvt_init(int P, const double* mean, const double* cov, double df, double* state, void* stream);
/* Enqueues `iters` pairs A, B of definition 2; trace holds max_iter doubles.  max_iter + 1 pairs always finish. */
int sgmcmc_fit_mvt_iterate(const void* w, int dtype, const sgmcmc_fit_geometry* geometry, int iters, int64_t max_iter,
                           double tol, double df_lo, double df_hi, double* part, int64_t* counts, double* state,
                           double* trace, void* stream);
/* Definition 3: out [5], zeros [1].  Two launches. */
int sgmcmc_fit_abs_stats(const void* w, int dtype, const sgmcmc_fit_geometry* geometry, double loc, double beta,
                         double* part, int64_t* counts, double* out, int64_t* zeros, void* stream);

/* ---- Goodness of fit of the fitted element-wise families (fp64, deterministic) ------------------------------------------
 * The question the fits of sgmcmc_fit_* were made for: which family the weights follow, and where a family fails.
 * This is the definition, restated in tests/gof_reference.py.
 * A RECORD is (family, shape, loc, scale), the parameters in scipy's order:
 *     SGMCMC_GOF_UNIFORM  on [loc, loc + scale]        (no shape)     the identity, which makes the sums testable exactly
 *     SGMCMC_GOF_NORM, SGMCMC_GOF_LAPLACE               (no shape)
 *     SGMCMC_GOF_T        shape = df    in [SGMCMC_GOF_DF_MIN, SGMCMC_GOF_DF_MAX]
 *     SGMCMC_GOF_GENNORM  shape = beta  in [SGMCMC_GOF_BETA_MIN, SGMCMC_GOF_BETA_MAX]
 *     SGMCMC_GOF_DGAMMA   shape = a     in [SGMCMC_GOF_A_MIN, SGMCMC_GOF_A_MAX]
 * loc finite, scale finite and > 0.  All arithmetic is fp64.
 *  1. The log-tail.  z = |x - loc| / scale; lt(z) = log T(z), T the probability beyond z on one side, formed in log space:
 *       norm     log(erfcx(z / sqrt 2) / 2) - z^2 / 2                laplace  log(1/2) - z
 *       t        T = I_x(df/2, 1/2) / 2, x = df / (df + z^2), I the regularised incomplete beta function by its
 *                continued fraction (of whichever tail converges; the upper tail's in its even part, written in x, 1 - x
 *                and (df + 1) (1 - x) / 2 - 1/2, each formed from z with one rounding), its prefactor x^(df/2)
 *                (1 - x)^(1/2) / B(df/2, 1/2) a logarithm in which only Stirling's remainders of the three lgamma appear
 *       gennorm  T = Q(1/beta, z^beta) / 2                           dgamma   T = Q(a, z) / 2
 *     Q(a, y) the regularised upper incomplete gamma function: 1 - P by P's series for y < a + 1, the continued fraction
 *     (modified Lentz) else; the prefactor y^a e^-y / Gamma(a) a logarithm, written a (log1p(u) - u) + log(a / 2 pi) / 2
 *     - D(a), u = (y - a) / a, D Stirling's remainder of lgamma(a).  z = 0 gives T = 1/2 exactly.  On the side of x:
 *     x > loc: 1 - F = T, log(1 - F) = lt, F = 1 - T, log F = log1p(-T); x < loc: the mirror image.  lt is finite where
 *     T underflows (lt down to about -1e300).  uniform: F = clamp((x - loc) / scale, 0, 1), log F = log(F),
 *     log(1 - F) = log1p(-F).  |z| >= 1e150 is taken as T = 0; a NaN gives NaN.
 *  2. The statistics of an ASCENDING array x_(1) <= ... <= x_(n) under a record, u_i = F(x_(i)):
 *       D+ = max_i (i / n - u_i)     D- = max_i (u_i - (i - 1) / n)     D = max(D+, D-), attained at the smallest such i
 *       (D+ where D+ >= D-);  W^2 = 1 / (12 n) + sum_i (u_i - (2 i - 1) / (2 n))^2;
 *       A^2 = -n - (1 / n) sum_i [(2 i - 1) log F_i + (2 (n - i) + 1) log(1 - F_i)]
 *     (the Anderson-Darling sum with its second factor re-indexed i -> n + 1 - i).  Summation order: tiles of
 *     SGMCMC_GOF_TILE consecutive values; workgroup b of min(tiles, SGMCMC_GOF_MAX_BLOCKS) takes tiles b, b + blocks, ...;
 *     thread t of 256 adds values t, t + 256, ... of each of its tiles in ascending order (compensated, Neumaier), the
 *     threads meet in the fixed tree t += t + 128, ..., t + 1 and the workgroups in ascending order (compensated).  A
 *     function of the sorted values and the records only.  Non-finite values are counted and left out.
 *     out, SGMCMC_GOF_OUT doubles per record: D, D+, D-, the 1-based index of the supremum, x there, W^2, A^2, the count
 *     of non-finite values.  A^2 is +inf when a value lies where a record's F is 0 or 1.
 *  3. Quantiles at p_j = (j - 1/2) / K, j = 1 .. K <= SGMCMC_GOF_MAX_QUANTILES: model [count][K], F^-1(p_j) = loc -+ scale z
 *     with lt(z) = log min(p, 1 - p) by Newton steps on lt kept inside a bracket, until a step is below 1e-10 z;
 *     empirical [K], numpy's linear rule on the ascending array: pos = (n - 1) p, lo = floor(pos), g = pos - lo,
 *     a = x[lo], b = x[min(lo + 1, n - 1)]; b - (b - a) (1 - g) for g >= 1/2, a + (b - a) g else, every operation rounded once.
 * 1 <= n <= 2^31 - 1, 1 <= count <= SGMCMC_GOF_MAX_RECORDS; anything else, a NULL pointer or a parameter outside its
 * range returns hipErrorInvalidValue and launches nothing.  Nothing is allocated, nothing synchronises. */
#define SGMCMC_GOF_MAX_RECORDS 6
#define SGMCMC_GOF_MAX_QUANTILES 4096
#define SGMCMC_GOF_TILE 1024
#define SGMCMC_GOF_MAX_BLOCKS 1024
#define SGMCMC_GOF_PART 8
#define SGMCMC_GOF_OUT 8
#define SGMCMC_GOF_UNIFORM 0
#define SGMCMC_GOF_NORM 1
#define SGMCMC_GOF_LAPLACE 2
#define SGMCMC_GOF_T 3
#define SGMCMC_GOF_GENNORM 4
#define SGMCMC_GOF_DGAMMA 5
#define SGMCMC_GOF_DF_MIN 0.1
#define SGMCMC_GOF_DF_MAX 1e4
#define SGMCMC_GOF_BETA_MIN 0.1
#define SGMCMC_GOF_BETA_MAX 10.0
#define SGMCMC_GOF_A_MIN 0.1
#define SGMCMC_GOF_A_MAX 1e4
typedef struct sgmcmc_gof_record {
  int32_t family, reserved;
  double shape, loc, scale;
} sgmcmc_gof_record;

/* Doubles of the workspace of sgmcmc_gof_statistics at n values; -1 for an n that is refused.  Host only. */
int64_t sgmcmc_gof_workspace_doubles(int64_t n);
/* Definition 1 at m points x (fp32 or fp64): out [4][m] = F, 1 - F, log F, log(1 - F).  One launch. */
int sgmcmc_gof_cdf(const void* x, int is_f64, int64_t m, const sgmcmc_gof_record* record, double* out, void* stream);
/* Definition 2 for `count` records at once: one pass in which every value is loaded once, and one workgroup that adds
 * the partials.  out [count][SGMCMC_GOF_OUT]. */
int sgmcmc_gof_statistics(const void* sorted, int is_f64, int64_t n, const sgmcmc_gof_record* records, int count,
                          double* workspace, double* out, void* stream);
/* Definition 3: model [count][K], empirical [K].  One launch. */
int sgmcmc_gof_ppf(const void* sorted, int is_f64, int64_t n, const sgmcmc_gof_record* records, int count, int K,
                   double* model, double* empirical, void* stream);

/* ---- The Rao-Blackwellised regression model: marginal likelihood of the last layer integrated out (fp64, deterministic) --
 * The reference's RaoBRegressionModel (models/base.py:194-311) gives the last layer an iid Normal(0, s2) prior and
 * integrates it out; what a sampler differentiates is the marginal likelihood below.  This is the definition, restated
 * in tests/raob_reference.py.  f [N, F] (fp32 or fp64, row-major) are the features of the N training rows, y [N] their
 * targets, s2 = last_layer_std^2, v = noise_std^2.  All arithmetic is fp64; f and y are widened as they are read.
 *     G = f^T f,  c = f^T y,  yy = y^T y,  A = s2 G + v I = L L^T,  w = L^-1 c,  b = L^-T w = A^-1 c
 *     log p(y | f) = -1/2 [N log 2 pi + (N - F) log v + yy / v + 2 sum_a log L_aa - (s2 / v) |w|^2]
 *     d/df, row n:   -s2 A^-1 f_n + (s2 / v) r_n b,   r_n = y_n - s2 f_n . b
 *     d/dv:          -1/2 [(N - F) / v - yy / v^2 + |L^-1|_F^2 + (s2 / v^2) |w|^2 + (s2 / v) |b|^2]     (|L^-1|_F^2 = tr A^-1)
 *     predictive at a row f*:  mean s2 f* . b,  variance v s2 |L^-1 f*|^2 + v  (never below v)
 * Summation order.  Gram: the rows are cut into tiles of SGMCMC_RAOB_TILE_ROWS; workgroup g of min(tiles,
 * SGMCMC_RAOB_MAX_BLOCKS) takes tiles g, g + blocks, ...  With y as column F, the lower triangle of order F + 1 is cut
 * into 4 x 4 blocks, nb = B (B + 1) / 2 of them, B = ceil((F + 1) / 4); a block is cut into S = 256 / nb row slices, slice q
 * adds rows q, q + S, ... of a tile from 0 by FMA, the tiles' sums are added in ascending order (compensated, Neumaier),
 * the slices from 0 in ascending order (compensated); the workgroups' partial records -- the packed lower triangle:
 * G's rows, then c, then yy, (F + 1)(F + 2) / 2 doubles -- are added in ascending order (compensated).  Factor: the
 * right-looking Cholesky, A_ik -= L_ij L_kj in ascending j, L_ij = A_ij / L_jj, and in the same sweep the forward
 * substitution X = L^-1: X_jc = X_jc / L_jj, X_ic -= L_ij X_jc in ascending j; multiplication and subtraction are
 * rounded separately.  w_a = sum_k X_ak c_k, b_a = sum_k X_ka w_k, (A^-1)_ab = sum_k X_ka X_kb, the sums of squares:
 * from 0 in ascending k, products and sums rounded separately.  The rows' dot products (gradient, predictive) are FMA
 * chains in ascending k; |L^-1 f*|^2 adds u_a^2 by FMA in 8 chains a = m, m + 8, ... that are added in ascending m.
 * The STATE RECORD, SGMCMC_RAOB_STATE_DOUBLES(F) doubles: SGMCMC_RAOB_SCALARS scalars {log p, d/dv, v, s2, log det A,
 * |w|^2 = c^T b, |b|^2, tr A^-1, yy, N, F, 0 ...}, then b [F], L^-1 [F][F], A^-1 [F][F], G [F][F], c [F], L [F][F]
 * (row-major, the triangles' other halves zero).  A pivot that is not > 0 or not finite makes every entry of the record
 * NaN except the sums G, c, yy and the sizes; the gradient and the predictive of such a record are NaN.  Nothing traps.
 * 1 <= N < 2^31, 1 <= F <= SGMCMC_RAOB_MAX_F; anything else or a NULL pointer returns hipErrorInvalidValue and launches
 * nothing.  The caller provides every buffer; nothing is allocated, nothing synchronises, no atomics. */
#define SGMCMC_RAOB_MAX_F 64
#define SGMCMC_RAOB_TILE_ROWS 64
#define SGMCMC_RAOB_MAX_BLOCKS 256
#define SGMCMC_RAOB_SCALARS 16
#define SGMCMC_RAOB_STATE_DOUBLES(F) (SGMCMC_RAOB_SCALARS + 2 * (F) + 4 * (F) * (F))
/* Doubles of the workspace (the workgroups' partial records) at N rows of F features; -1 when refused.  Host only. */
int64_t sgmcmc_raob_workspace_doubles(int64_t N, int F);
/* The Gram pass: one launch that reads f once and writes the partial records. */
int sgmcmc_raob_gram(const void* f, const void* y, int is_f64, int64_t N, int F, double* workspace, void* stream);
/* One workgroup: the partials -> the state record.  v is read from noise_var_device [1] (device memory) when that is
 * not NULL, so that a noise variance that lives on the device never visits the host; else it is noise_var. */
int sgmcmc_raob_factor(const double* workspace, int64_t N, int F, double last_layer_var, double noise_var,
                       const double* noise_var_device, double* state, void* stream);
/* grad_f [N, F] (f's dtype) = upstream d log p / d f and, unless NULL, grad_noise_var [1] = upstream d log p / dv;
 * upstream [1] is in device memory and of f's dtype (NULL: 1).  One launch. */
int sgmcmc_raob_grad(const void* f, const void* y, int is_f64, int64_t N, int F, const double* state,
                     const void* upstream, void* grad_f, double* grad_noise_var, void* stream);
/* mean [M], var [M] of the predictive at the rows of f_star [M, F] (1 <= M < 2^31).  One launch. */
int sgmcmc_raob_predict(const void* f_star, int is_f64, int64_t M, int F, const double* state, double* mean,
                        double* var, void* stream);

/* ---- Sampler temperature diagnostics: chi-square laws of the kinetic temperatures (fp64, deterministic) ---------------
 * A parameter tensor with d elements has kinetic temperature estimate T^ with T^ / T ~ chi^2_d / d at the target T (the
 * reference reads them off plots: bnn_priors/plot.py:14-141).  With a = d / 2 and r = T^ / T the distribution function is
 * the regularised incomplete gamma function P(a, a r), Q = 1 - P.  d is an integer in [1, 2^31 - 1]; a d outside it gives
 * NaN.  Restated at 50 digits in tests/temperature_reference.py; the methods, their switch points
 * (SGMCMC_TEMPER_UNIFORM_A, SGMCMC_TEMPER_UNIFORM_U) and the measured error on each side are in csrc/temper_hip.inc.
 *  1. Tails.  est [S, K] (fp32 or fp64, element (s, k) at s * stride_s + k * stride_k), r = est / temperature[s *
 *     temp_stride] (temperature in device memory; temp_stride = 0 for one value; NULL: r = est), sizes [K] int64 in device
 *     memory.  out [4][S * K]: P, Q, log P, log Q.  One of the two tails is evaluated in log space and the other derived
 *     from it; r <= 0 gives P = 0, r = inf gives Q = 0, NaN gives NaN.
 *  2. Quantiles.  out [K][M]: the r at which the tail (upper[m] ? Q : P) of tensor k equals value[m] (its logarithm when
 *     is_log): Newton steps on the log-tail from the Wilson-Hilferty point inside a bracket, 100 at most.  value, upper in
 *     device memory.  A value outside [0, 1] gives NaN, 0 and 1 the ends 0 and inf.
 *  3. The step table.  bounds [K][C][2] (lower, upper), C <= SGMCMC_TEMPER_MAX_LEVELS.  share [C][S]: the number of
 *     tensors with lower <= r <= upper, both ends included, NaN and inf outside, divided by K.  totals [K * C + 1] int64:
 *     per tensor and level the number of steps inside, then the number of finite r: integer counts, exact in any order.
 *     Workgroup b of min(ceil(S / 256), 256) takes the tiles of 256 steps b, b + blocks, ...; its counts are gathered in
 *     LDS (K * C + 1 <= 4096; else in memory directly) and added to totals by integer atomics.
 *     mean [S], se [S]: with w = sizes and x = est (NOT divided by the temperature), Cochran's (1977) weighted mean
 *     xw = sum w x / sum w and se = K / ((K - 1) (sum w)^2) [sum (w x - wb xw)^2 - 2 xw sum (w x - wb xw)(w - wb)
 *     + xw^2 sum (w - wb)^2], wb = sum w / K.  The bracket equals sum w^2 (x - xw)^2 identically and is evaluated in
 *     that form (the three terms cancel); every sum runs over k ascending, compensated (Neumaier).  C = 0 computes
 *     mean and se only (temperature, bounds, share, totals unused); mean = se = NULL computes the coverage only.
 *  4. EWMA.  x [R, S] strided, y [R][S]: y_0 = x_0, y_t = (1 - alpha) x_t + alpha y_(t-1), 0 <= alpha < 1, products and
 *     sum rounded separately.  One workgroup per row; thread t of SGMCMC_TEMPER_SCAN owns the L = ceil(S / SCAN) steps
 *     from t L on, composes their affine maps in order, the composites are scanned (Hillis-Steele) and the steps replayed
 *     from the carry.  alpha = 0 copies the input's bits; a NaN poisons what follows it in its own row and nothing else;
 *     +-inf stays +-inf in what follows it, as step by step (also where alpha^L underflows).
 * 1 <= S, S * K <= 2^31 - 1 (S * R for the EWMA); anything else or a missing pointer returns hipErrorInvalidValue and
 * launches nothing.  The caller provides every buffer; nothing is allocated, nothing synchronises, and the only atomics
 * are the integer counts of 3. */
#define SGMCMC_TEMPER_SCAN 256
#define SGMCMC_TEMPER_MAX_LEVELS 16
#define SGMCMC_TEMPER_UNIFORM_A 100.0
#define SGMCMC_TEMPER_UNIFORM_U 0.3
int sgmcmc_temper_tails(const void* est, int is_f64, int64_t S, int K, int64_t stride_s, int64_t stride_k,
                        const double* temperature, int64_t temp_stride, const int64_t* sizes, double* out, void* stream);
int sgmcmc_temper_quantile(const int64_t* sizes, int K, const double* value, const int32_t* upper, int M, int is_log,
                           double* out, void* stream);
int sgmcmc_temper_steps(const void* est, int is_f64, int64_t S, int K, int64_t stride_s, int64_t stride_k,
                        const double* temperature, int64_t temp_stride, const int64_t* sizes, const double* bounds, int C,
                        double* share, double* mean, double* se, int64_t* totals, void* stream);
int sgmcmc_temper_ewma(const void* x, int is_f64, int R, int64_t S, int64_t stride_r, int64_t stride_s, double alpha,
                       double* y, void* stream);

/* ---- Correlation between the variables of a stack of weight samples (fp64, deterministic) ------------------------------
 * The second half of the study of trained weights: are the rows, the columns or the channels of a layer correlated, and
 * compared with what null.  This is the definition, restated in tests/weight_correlation_reference.py.
 * Stack and geometry.  A stack w [S, *shape] (fp32 or fp64, any strided view) is read in place.  One axis of `shape` holds
 * the V VARIABLES (variable v at v * v_stride elements); every other axis, S included, indexes the n = S numel(shape) / V
 * OBSERVATIONS, numbered k = 0 .. n - 1 row-major over the remaining axes in their original order: up to four observation
 * dimensions (size, stride in elements; unused ones are size 1, neighbours that one stride walks are merged).  v_major != 0
 * tells the loader that v_stride is below the innermost observation stride, so that a tile is walked variable-first
 * (coalesced along the stack's fastest dimension); it changes no result.  The Gram entry point takes a leading batch of R
 * such matrices, matrix r at r * batch_stride elements (R = 1 for a stack; R > 1 for permuted replicates [R][V][n]).
 * Quantities, all fp64, every operation rounded once:
 *     m_v = x_v(0) + (sum_k (x_v(k) - x_v(0))) / n   (the mean, summed about the first observation: two passes, so that a
 *           variable 10^4 standard deviations from 0 keeps its digits and a constant variable has d = 0 exactly)
 *     d = x - m;   G = d d^T;   cov = G / (n - ddof);   corr_ij = G_ij / sqrt(G_ii G_jj).
 * A variable with G_vv = 0 is flagged in zero_variance; its cov row and column are 0, its corr row and column NaN, and it
 * leaves the off-diagonal statistics.  A non-finite element anywhere makes mean, cov and corr NaN (zero_variance 0);
 * nonfinite[0] counts the elements.
 * Summation order, a function of (V, n) and of the workspace alone (whatever the strides): observations are cut into
 * chunks of SGMCMC_CORR_CHUNK.  Mean: workgroup `seg` of sgmcmc_corr_mean_blocks() takes chunks seg, seg + blocks, ...;
 * slot q = 0 .. 3 of a variable adds observations q, q + 4, ... of a chunk from 0 in ascending order, the chunks' sums are
 * added in ascending order (compensated, Neumaier), the four slots ((0 + 1) + 2) + 3, the workgroups' partials in
 * ascending order (compensated).  Gram: G is cut into SGMCMC_CORR_TILE^2 blocks, of which the upper triangle is formed;
 * workgroup `split` of sgmcmc_corr_splits() takes chunks split, split + splits, ... and accumulates them on the fp64
 * matrix pipe (v_mfma_f64_16x16x4_f64: four observations per instruction, in the instruction's order, chunk after chunk
 * in one accumulator); the finish adds the splits from 0 in ascending order and mirrors the triangle.  splits =
 * min(chunks, SGMCMC_CORR_MAX_SPLITS, SGMCMC_CORR_TARGET_BLOCKS / block pairs, workspace_bytes / (8 V^2)): it does not
 * depend on R, so a batch gives the bits of R single calls; the slabs take splits * R * V^2 doubles.
 * Off-diagonal statistics of a correlation matrix [V][V], over the pairs i < j of variables whose diagonal entry is not
 * NaN (their entries are taken as they are): stats [SGMCMC_CORR_STATS] = {mean r, mean |r|, rms r = sqrt(mean r^2),
 * max |r|, sum r^2}, all NaN when there is no pair; counts [3] = {pairs, i, j of max |r|: the smallest (i, j) in row-major
 * order on a tie, (-1, -1) without a pair}.  One workgroup per matrix: thread t adds the pairs (i, i + 1 + t + 256 a),
 * rows then columns ascending (compensated), then the fixed tree (t += t + 128, ..., t + 1).
 * No floating-point atomics; two calls give the same bits.  The caller provides every buffer (part: blocks * V doubles,
 * counts: ceil(V / TILE) * blocks int64); nothing is allocated, nothing synchronises.  Limits: 1 <= V <=
 * SGMCMC_CORR_MAX_V, 2 <= n < 2^31, 0 <= ddof < n, strides >= 0, the product of the sizes = n, 1 <= R <=
 * SGMCMC_CORR_MAX_BATCH, 1 <= splits <= min(chunks, SGMCMC_CORR_MAX_SPLITS); anything else or a missing pointer returns
 * hipErrorInvalidValue and launches nothing. */
#define SGMCMC_CORR_TILE 64
#define SGMCMC_CORR_CHUNK 32
#define SGMCMC_CORR_MAX_V 1024
#define SGMCMC_CORR_MAX_SPLITS 64
#define SGMCMC_CORR_TARGET_BLOCKS 1024
#define SGMCMC_CORR_MEAN_BLOCKS 512
#define SGMCMC_CORR_MAX_BATCH 65535
#define SGMCMC_CORR_STATS 5
typedef struct sgmcmc_corr_geometry {
  int32_t V, v_major;
  int64_t n;
  int64_t v_stride;
  int64_t size[4], stride[4];
} sgmcmc_corr_geometry;

/* Workgroups per block pair of the Gram pass (0: workspace_bytes holds no V^2 doubles; -1: a refused shape). */
int sgmcmc_corr_splits(int V, int64_t n, int64_t workspace_bytes);
/* Workgroups per variable tile of the mean pass = min(chunks, SGMCMC_CORR_MEAN_BLOCKS / ceil(V / TILE)); -1 if refused. */
int sgmcmc_corr_mean_blocks(int V, int64_t n);
/* mean [V], nonfinite [1].  Two launches. */
int sgmcmc_corr_mean(const void* w, int dtype, const sgmcmc_corr_geometry* geometry, double* part, int64_t* counts,
                     double* mean, int64_t* nonfinite, void* stream);
/* slabs [splits][R][V][V], of which the blocks of the upper triangle are written.  mean [V] is shared by the batch. */
int sgmcmc_corr_gram(const void* x, int dtype, const sgmcmc_corr_geometry* geometry, int R, int64_t batch_stride,
                     const double* mean, int splits, double* slabs, void* stream);
/* cov (may be NULL), corr [R][V][V], zero_variance [R][V] (bytes); nonfinite (may be NULL) as sgmcmc_corr_mean wrote it. */
int sgmcmc_corr_finish(const double* slabs, int splits, int R, int V, int64_t n, int ddof, const int64_t* nonfinite,
                       double* cov, double* corr, uint8_t* zero_variance, void* stream);
/* stats [R][SGMCMC_CORR_STATS], counts [R][3] of the R matrices corr [R][V][V]. */
int sgmcmc_corr_offdiag(const double* corr, int R, int V, double* stats, int64_t* counts, void* stream);

/* ---- Kernel Stein discrepancy and Stein thinning (fp64, deterministic) ------------------------------------------------------
 * Do the draws target the right distribution?  The kernel Stein discrepancy with the inverse multiquadric kernel (Gorham &
 * Mackey 2017) needs the draws and the gradient of the log target at each draw only.  This is the definition, restated in
 * tests/stein_reference.py.
 * Inputs: the samples X [S][D] and the scores G [S][D], g_i = grad log p(x_i), both fp32 or both fp64, unit column stride
 * and any row stride (x_stride, score_stride, in elements).  Parameters c^2 > 0 and -1 < beta < 0; d is the total dimension
 * (D, or the sum over the tensors of a dict whose Gram matrices were added).
 * Anchor: x~_i = x_i - x_0, subtracted in fp64 by the loader (exact for fp32 input): everything below depends on X through
 * differences only, so a common offset of the samples costs no digits.
 * Gram pass, on the fp64 matrix pipe: the symmetric Gram matrix gram [2S][2S] of the 2S rows [X~; G], i.e.
 *     A = X~ X~^T = gram[i][j],   B = X~ G^T, B_ij = x~_i . g_j = gram[i][S + j],   C = G G^T = gram[S + i][S + j].
 * Stein matrix, entry (i, j) evaluated with i <= j and mirrored (K and r2 are symmetric bit for bit):
 *     r2_ij = max(0, (A_ii + A_jj) - 2 A_ij)                        (exactly 0 on the diagonal)
 *     t_ij  = ((B_ii - B_ij) - B_ji) + B_jj                         = (g_i - g_j) . (x_i - x_j)
 *     u = c^2 + r2_ij;   p0 = u^beta (1 / sqrt(u) for beta = -1/2, else pow);   p1 = p0 / u;   p2 = p1 / u
 *     K_ij  = (p0 C_ij - 2 beta p1 (t_ij + d)) - 4 beta (beta - 1) p2 r2_ij
 * K is positive semi-definite up to rounding.  A NaN or Inf anywhere in X or G is counted in nonfinite[0] and makes K, r2
 * and every statistic NaN.
 * Statistics of K [S][S] and a batch of weight vectors W [R][S] (W = NULL: R = 1 vector of ones, by the same arithmetic, so
 * that W = 1 gives v_stat bit for bit):
 *     rowsum_ri = sum_j W_rj K_ij;   row_mean = rowsum / S;   Q_r = sum_i W_ri rowsum_ri / S^2   (v_stat for W = 1)
 *     stats [R][SGMCMC_STEIN_STATS] = {Q_r, (sum_i W_ri rowsum_ri - sum_i W_ri^2 K_ii) / (S (S - 1)), Q_r < 0 ? 0 : sqrt(Q_r)}
 *     = {v_stat, u_stat, ksd} for W = 1.
 * Thinning (Riabiz et al. 2022): pi_1 = argmin_j K_jj / 2, pi_m = argmin_j [K_jj / 2 + sum_{a < m} K(pi_a, j)]; picks may
 * repeat, ties go to the smaller index, a NaN objective never wins;  total_m = total_{m-1} + (2 sum_{a < m} K(pi_a, pi_m) +
 * K(pi_m, pi_m)),  path_m = sqrt(total_m) / m.
 * Summation order, a function of (S, D) and of the workspace alone (whatever the row strides): coordinates are cut into
 * chunks of SGMCMC_STEIN_CHUNK; gram is cut into SGMCMC_STEIN_TILE^2 blocks of which the upper triangle is formed; workgroup
 * `split` of sgmcmc_stein_splits() takes chunks split, split + splits, ... and accumulates them on the fp64 matrix pipe
 * (v_mfma_f64_16x16x4_f64: four coordinates per instruction, chunk after chunk in one accumulator); sgmcmc_stein_reduce adds
 * the splits from 0 in ascending order and mirrors the triangle.  splits = min(chunks, SGMCMC_STEIN_MAX_SPLITS,
 * SGMCMC_STEIN_TARGET_BLOCKS / block pairs, workspace_bytes / (8 (2S)^2)).  Row sums: lane l of a wave adds j = l, l + 64,
 * ... ascending, then the fixed tree (l += l + 32, ..., l + 1); forms: thread t adds i = t, t + 256, ... ascending, then the
 * fixed tree (t += t + 128, ..., t + 1); neither depends on R, so a batch gives the bits of R single calls.  The thinning
 * walk is one workgroup with the running sums in LDS and exactly m trips of a fixed-tree arg-min over (value, index).
 * No floating-point atomics, no waiting between workgroups; two calls give the same bits.  The caller provides every buffer
 * (slabs: splits (2S)^2 doubles; counts: splits ceil(2S / TILE) int64; rowsum: R S doubles); nothing is allocated, nothing
 * synchronises.  Limits: 2 <= S <= SGMCMC_STEIN_MAX_S, 1 <= D < 2^31, strides >= 0, 1 <= splits <= min(chunks,
 * SGMCMC_STEIN_MAX_SPLITS), 1 <= R <= SGMCMC_STEIN_MAX_BATCH, 1 <= m <= SGMCMC_STEIN_MAX_PICKS, d >= 1; anything else or a
 * missing pointer returns hipErrorInvalidValue and launches nothing. */
#define SGMCMC_STEIN_TILE 64
#define SGMCMC_STEIN_CHUNK 32
#define SGMCMC_STEIN_MAX_S 1024
#define SGMCMC_STEIN_MAX_SPLITS 64
#define SGMCMC_STEIN_TARGET_BLOCKS 1024
#define SGMCMC_STEIN_MAX_BATCH 65535
#define SGMCMC_STEIN_STATS 3
#define SGMCMC_STEIN_MAX_PICKS 1048576

/* Workgroups per block pair of the Gram pass (0: workspace_bytes holds no (2S)^2 doubles; -1: a refused shape). */
int sgmcmc_stein_splits(int S, int64_t D, int64_t workspace_bytes);
/* slabs [splits][2S][2S], of which the blocks of the upper triangle are written; counts [splits][ceil(2S / TILE)]. */
int sgmcmc_stein_gram(const void* x, const void* score, int dtype, int S, int64_t D, int64_t x_stride, int64_t score_stride,
                      int splits, double* slabs, int64_t* counts, void* stream);
/* gram [2S][2S] (every entry), nonfinite [1]. */
int sgmcmc_stein_reduce(const double* slabs, const int64_t* counts, int splits, int S, double* gram, int64_t* nonfinite,
                        void* stream);
/* K [S][S] and r2 [S][S] (either may be NULL) of a gram matrix, or of a sum of them; c2_device (may be NULL) overrides c2. */
int sgmcmc_stein_finish(const double* gram, int S, double d, double c2, const double* c2_device, double beta,
                        const int64_t* nonfinite, double* K, double* r2, void* stream);
/* rowsum [R][S], row_mean [R][S] (may be NULL), stats [R][SGMCMC_STEIN_STATS]; W [R][S] or NULL (then R = 1).  Two launches. */
int sgmcmc_stein_forms(const double* K, int S, const double* W, int R, double* rowsum, double* row_mean, double* stats,
                       void* stream);
/* indices [m], path [m]. */
int sgmcmc_stein_thin(const double* K, int S, int m, int64_t* indices, double* path, void* stream);

/* ---- Lanczos, tridiagonal eigenvalues and the effective dimensionality (fp64, deterministic) --------------------------------
 * How many directions of weight space do the data determine?  N_eff(alpha) = sum_i lambda_i / (lambda_i + alpha) over the
 * positive eigenvalues of a Hessian (MacKay 1992; Maddox et al. 2020), from the Ritz values of m Lanczos steps with full
 * reorthogonalisation.  The matrix-vector product is the caller's.  This is the definition, restated in
 * tests/eff_dim_reference.py.
 * One step, given the orthonormal rows V_0 .. V_j of V (fp64, unit column stride, any row stride v_stride in elements) and
 * w = A V_j (fp64, contiguous, updated in place):
 *     pass p = 1, 2:   c_k = V_k . w  for k = 0 .. j  (sgmcmc_lanczos_dots, sgmcmc_lanczos_reduce with pass = p - 1), then
 *                      w <- w - sum_k c_k V_k, k ascending, one fma per term       (sgmcmc_lanczos_update, mode 0)
 *     alpha_j = c_j(1) + c_j(2);   beta_j = sqrt(w . w) after the second pass;   scale = max(scale, |alpha_j|, beta_j)
 *     no breakdown:  beta_j > rtol scale.  Then V_j+1 = w (1 / beta_j) (sgmcmc_lanczos_update, mode 1), else beta_j is
 *     written as exactly 0 and state[3] = 1: the host puts a fresh vector into w and runs the same calls with restart = 1
 *     (no alpha, beta, scale; no breakdown: the norm after > rtol times the norm before the two passes).
 * state [SGMCMC_LANCZOS_STATE] doubles: {scale, 1 / beta, beta, breakdown (0 / 1), non-finite elements of w seen so far, the
 * norm of w before the first pass}; the caller zeroes it once.  coef [2][SGMCMC_LANCZOS_MAX_M]: the c of the two passes.
 * Summation order, a function of (D, workspace_bytes) alone: coordinates are cut into chunks of SGMCMC_LANCZOS_CHUNK, one
 * coordinate per thread; workgroup `split` of sgmcmc_lanczos_splits() = min(chunks, SGMCMC_LANCZOS_MAX_SPLITS,
 * workspace_bytes / (8 SGMCMC_LANCZOS_WIDTH)) takes chunks split, split + splits, ..., a thread adds its coordinate of them in
 * that order (fma), lane l of a wave adds lane l + 32, ..., l + 1, the four waves are added from 0, and the reduce launch
 * adds the workgroups from 0.  Neither the row stride nor j enters; no floating-point atomics; two calls give the same bits.
 * ws: splits rows of SGMCMC_LANCZOS_WIDTH doubles {c_0 .. c_MAX_M-1, w . w, non-finite}: sgmcmc_lanczos_workspace_bytes().
 * sgmcmc_tridiag_eig: `batch` symmetric tridiagonal matrices (diagonal alpha[b ld + i], off-diagonal beta[b ld + i], i < m - 1)
 * by implicit QL with Wilkinson shifts, one workgroup each, d, e and a sweep's rotations in LDS; work [batch][m][m] holds the
 * eigenvector matrix transposed while it is rotated.  theta[b ld + p] ascending (ties by original index), Y [batch][m][m]
 * with column p the eigenvector of theta_p, sweeps[b], failed[b] = 1 (and NaN outputs) if an eigenvalue is not deflated after
 * SGMCMC_TRIDIAG_MAX_SWEEPS sweeps or is NaN.  e_i is negligible when |e_i| <= eps (|d_i| + |d_i+1|).
 * sgmcmc_lanczos_ritz: U [D][k] = V^T Y[:, col0 .. col0 + k) on the fp64 matrix pipe (v_mfma_f64_16x16x4_f64), the sum over
 * the m rows in ascending groups of four; column j is multiplied by -1 where Y[0][col0 + j] < 0 and, with positive != 0, set
 * to exact zeros where theta[col0 + j] <= m eps max(|theta_0|, |theta_m-1|).
 * sgmcmc_effdim: out[b][a] = sum over eigs[b][i] > 0 of eigs / (eigs + alphas[a]) by compensated sums (thread t of 256 adds
 * i = t, t + 256, ..., thread 0 adds the threads from 0); nonpos[b], nonfinite[b] count the finite entries <= 0 and the NaN /
 * Inf entries, which are left out.
 * Limits: 1 <= D < 2^31, 1 <= rows, m <= SGMCMC_LANCZOS_MAX_M, 1 <= splits <= min(chunks, SGMCMC_LANCZOS_MAX_SPLITS), batch,
 * A <= SGMCMC_LANCZOS_MAX_BATCH; anything else or a missing pointer returns hipErrorInvalidValue and launches nothing.  The
 * caller provides every buffer; nothing is allocated and nothing synchronises. */
#define SGMCMC_LANCZOS_CHUNK 256
#define SGMCMC_LANCZOS_ROWS 16
#define SGMCMC_LANCZOS_MAX_M 512
#define SGMCMC_LANCZOS_MAX_SPLITS 512
#define SGMCMC_LANCZOS_MAX_BATCH 65535
#define SGMCMC_LANCZOS_WIDTH 514
#define SGMCMC_LANCZOS_STATE 8
#define SGMCMC_TRIDIAG_MAX_SWEEPS 60

/* Workgroups along D of the step kernels (0: workspace_bytes holds no row of partials; -1: a refused shape). */
int sgmcmc_lanczos_splits(int64_t D, int64_t workspace_bytes);
/* Bytes of ws for that many workgroups (-1: a refused shape). */
int64_t sgmcmc_lanczos_workspace_bytes(int64_t D, int64_t workspace_bytes);
/* ws[split][k] = partial V_k . w, k < rows; ws[split][MAX_M] = partial w . w; ws[split][MAX_M + 1] = non-finite elements. */
int sgmcmc_lanczos_dots(const double* V, int64_t v_stride, int rows, const double* w, int64_t D, int splits, double* ws,
                        void* stream);
/* pass 0 / 1: coef[pass][k], k < rows; pass 2: alpha[j], beta[j] (unless restart) and state. */
int sgmcmc_lanczos_reduce(const double* ws, int splits, int rows, int pass, int j, int restart, double rtol, double* coef,
                          double* alpha, double* beta, double* state, void* stream);
/* mode 0: w -= sum_k coef[k] V_k and ws[split][MAX_M] = partial w . w afterwards; mode 1: v_next [D] = w * state[1]. */
int sgmcmc_lanczos_update(const double* V, int64_t v_stride, int rows, double* w, int64_t D, int splits, const double* coef,
                          int mode, const double* state, double* v_next, double* ws, void* stream);
int sgmcmc_tridiag_eig(const double* alpha, const double* beta, int batch, int m, int64_t ld, double* theta, double* Y,
                       double* work, int* sweeps, int* failed, void* stream);
int sgmcmc_lanczos_ritz(const double* V, int64_t v_stride, int m, int64_t D, const double* Y, const double* theta, int col0,
                        int k, int positive, double* U, void* stream);
int sgmcmc_effdim(const double* eigs, int64_t B, int k, const double* alphas, int A, double* out, int64_t* nonpos,
                  int64_t* nonfinite, void* stream);

/* Test hook: out[i] = spec normal (fp32) of noise index start+i. */
int sgmcmc_debug_normals(float* out, int64_t start, int64_t n, uint64_t seed, uint32_t stream,
                         uint64_t draw, uint32_t purpose, void* stream_);

#ifdef __cplusplus
}
#endif
#endif /* SGMCMC_HIP_H */
