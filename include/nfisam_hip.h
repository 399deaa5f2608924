/*
 * nfisam_hip.h — C ABI of the MI355X (gfx950) implementation of NF-iSAM's per-clique
 * normalizing-flow hot path (autoregressive rational-quadratic neural spline flow).
 *
 * The reference (MarineRoboticsGroup/NF-iSAM) has no FFI for this path: its boundary is the
 * Python module surface `flows.*` + the solver hooks of `slam.NFiSAM`.  This
 * header is what a binding for that surface links against; `nf-isam_amd/nfisam_hip/` is the
 * ctypes binding and INTEGRATION.md shows the stub a reference maintainer would add.  Each
 * entry point cites the reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *  - All `float*`/`uint8_t*` data arguments are DEVICE pointers (HBM), contiguous, row-major,
 *    borrowed for the duration of the enqueued work.  `int32_t* map` of the layout helper and
 *    everything documented "host" are host pointers.
 *  - `stream` is a `hipStream_t` passed as `void*` (0 = the null stream).  Work is enqueued
 *    on it; no entry point synchronises with the host unless its comment says so.
 *  - Return value: NFISAM_OK or an error code below; on NFISAM_ERR_LAUNCH the HIP error is
 *    left readable through `nfisam_last_hip_error()`.
 *  - No global mutable state except the last-error word; re-entrant across streams/devices.
 *  - There is NO CPU fallback anywhere behind this ABI.
 *
 * Symbols: n particles, D clique dimension (columns = [obs | separator | frontal]),
 * Ds leading columns that are given in conditional sampling, K spline bins (`num_knots`),
 * H hidden width, Po = 3K-1, B tail bound (5.0 in the reference, flows.py:51), L flow layers.
 *
 * Parameter storage ("kernel layout", float32, one block of `nfisam_nsf_kparam_count`
 * floats per flow layer, layers concatenated):
 *     init_param[PoP]
 *     for i = 1..D-1:  W0t[i][H]  b0[H]  W1t[H][H]  b1[H]  W2t[H][PoP]  b2[PoP]
 * where W*t are the TRANSPOSES ([in][out]) of the reference's nn.Linear weights
 * (flows.py:31-37), so that every weight row a wavefront consumes is contiguous (16-byte
 * aligned rows: scalar loads or ds_read_b128).  The PoP = 2*HP output columns are two halves,
 *     [ K width logits  | first floor(K/2) derivative logits | 0-pad to HP ]
 *     [ K height logits | remaining derivative logits        | 0-pad to HP ],  HP = 4*ceil((K + floor(K/2))/4)
 * (the reference's order is widths | heights | derivatives, flows.py:84-88): the two lanes that share
 * a particle in the training kernel each own one half.  Padding entries are zero and stay zero under training.
 * `nfisam_nsf_layout_map` gives the permutation to/from the reference's parameter order
 * (init_param, layers.{i-1}.network.{0,2,4}.{weight,bias}; flows.py:57-59).
 */
#ifndef NFISAM_HIP_H
#define NFISAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFISAM_OK 0
#define NFISAM_ERR_ARG 1          /* bad shape / NULL pointer / unsupported (K,H)  (ValueError) */
#define NFISAM_ERR_LAUNCH 2       /* HIP launch or runtime failure                              */
#define NFISAM_ERR_DOMAIN 3       /* numerical domain error flagged by a kernel (utils.py:74-76,133) */
#define NFISAM_ERR_NO_DEVICE 4    /* no usable gfx950 device                                    */
#define NFISAM_ERR_STALL 5        /* a chunk-persistent training launch gave up waiting for a block of its own that never
                                   * became resident (another process or launch held its place): the plan's parameters,
                                   * moments and loss record are those of an INCOMPLETE chunk -- not a numerical failure.
                                   * The library takes the one-launch-per-iteration graph for every later run of the
                                   * process; the caller re-runs the fit from its initial state (ABI 1400)          */

typedef void* nfisam_stream_t;

/* ABI version of this header (major*1000 + minor). */
int nfisam_abi_version(void);
/* Last HIP error code recorded by a failing call on this thread (0 if none). */
int nfisam_last_hip_error(void);
/* 1 if flows with (num_knots K, hidden_dim H) run on the kernels, else 0: K in 2..16, H in 1..16.  The kernels are
 * instantiated for H in {4, 8, 16}; every other width runs as the next compiled width with zero-padded hidden units (the
 * reference takes any width, src/flows/flows.py:26-41): a padded unit has zero in-weights, bias and out-weights, so its
 * activation is tanh(0) = 0 and every gradient touching it is an exact 0 -- Adam leaves the padding at zero (ABI 1500). */
int nfisam_nsf_supported(int K, int H);

/* ---- layout (host-only helpers, no GPU needed) ---------------------------------------- */
/* Parameters per layer in the reference's order = numel of NSF_AR.parameters() (flows.py:51-60). */
size_t nfisam_nsf_param_count(int D, int K, int H);
/* Floats per layer in kernel layout (>= param_count because of padding; for a hidden_dim that is not a compiled width:
 * the count of the next compiled width). */
size_t nfisam_nsf_kparam_count(int D, int K, int H);
/* host: map[kidx] = index into the reference-order blob, or -1 for padding. map has kparam_count entries. */
int nfisam_nsf_layout_map(int D, int K, int H, int32_t* map);

/* ---- inference ------------------------------------------------------------------------ */
/* NSF_AR.forward chained over L layers + prior log-prob (flows.py:65-93, models.py:11-24),
 * in the CORRECT layout (the reference returns a scrambled one).
 *   x[n,D] -> z[n,D] (nullable), logdet[n] (nullable), logprob[n] (nullable)
 *   logprob = -0.5|z|^2 - D/2 log(2 pi) + logdet
 * layer_stride: floats between consecutive layers' parameter blocks; 0 = kparam_count(D).  Because
 * the flow is autoregressive and dim i's block only depends on i, the first D' < D_model dims of a
 * trained D_model-dimensional flow ARE its D'-dimensional marginal flow: pass D = D' and
 * layer_stride = kparam_count(D_model) to evaluate it in place
 * (NormalizingFlowModelWithSeparator.separator_forward, slam/NFiSAM.py:157-173).  The same argument
 * exists on nfisam_nsf_inverse and nfisam_nsf_backward.                                     */
int nfisam_nsf_forward(const float* x, const float* kparams, int n, int D, int K, int H, float B,
                       int L, size_t layer_stride, float* z, float* logdet, float* logprob,
                       nfisam_stream_t stream);

/* NSF_AR.inverse / inverse_given_separator (flows.py:95-137) fused with the adapter's
 * normalisation of the given columns and un-normalisation + angle wrap of the result
 * (NormalizingFlowModelWithSeparator.{normalize_samples,inverse_given_separator,
 *  unnormalize_samples}, slam/NFiSAM.py:96-118,140-155).
 *   z[n,D-Ds] latent draws; x_sep[n,Ds] RAW (un-normalised) given columns, NULL iff Ds==0
 *   mean[D], std[D], circular[D] (1 = angle column): NULL mean => data already normalised and
 *   the output is left normalised (plain NSF_AR.inverse_given_separator).
 *   x_out[n,D-Ds]; logdet[n] nullable (sum of -log|dz/dx| over the solved columns, as NSF_AR.inverse)
 * L > 1 with given columns: layer l is conditioned on the given columns pushed through the marginal flow of
 * layers 0..l-1, so that forward(cat(x_sep, x_out)) returns z.  (The reference's literal loop feeds every layer
 * the raw columns, slam/NFiSAM.py:151-152, which inverts no composition; with flow_number = 1, its default, the
 * two coincide.)                                                                                              */
int nfisam_nsf_inverse(const float* z, const float* x_sep, const float* kparams, int n, int D, int Ds,
                       int K, int H, float B, int L, size_t layer_stride, const float* mean, const float* std,
                       const uint8_t* circular, float* x_out, float* logdet, nfisam_stream_t stream);

/* Elementwise rational-quadratic spline with per-element logits (flows.utils.unconstrained_RQS and
 * RQS, src/flows/utils.py:25-164).  inputs[M], widths[M,K], heights[M,K];
 * padded_derivatives=1: derivs[M,K-1], end slopes fixed to 1 and identity outside the box
 *                       (unconstrained_RQS with left=bottom=-tail_bound, right=top=tail_bound);
 * padded_derivatives=0: derivs[M,K+1] (bounded RQS; callers validate the domain, utils.py:74-76).
 * out[M], logabsdet[M].  Any K >= 1 with 1e-3*K <= 1 (utils.py:80-83).                      */
int nfisam_rqs(const float* inputs, const float* widths, const float* heights, const float* derivs, int M, int K,
               int inverse, float left, float right, float bottom, float top, int padded_derivatives,
               float* out, float* logabsdet, nfisam_stream_t stream);

/* ---- posterior traversal ------------------------------------------------------------------ */
/* One clique of the tree walk, parents before children.  Column indices refer to the sample matrix. */
typedef struct nfisam_post_clique {
    const float* kparams;        /* the clique's trained flow, kernel layout, D_model dims, L layers   */
    const float* mean;           /* [D_model] normalisation constants (slam/NFiSAM.py:515-548)        */
    const float* std;
    const uint8_t* circular;     /* [D_model] 1 = angle column                                        */
    int32_t D_model;             /* n_obs + all clique variable dims                                  */
    int32_t n_obs;               /* leading true-observation columns                                  */
    int32_t n_sep;               /* separator columns (already sampled by ancestors)                  */
    int32_t n_frontal;           /* columns sampled by this clique                                    */
    int32_t obs_off;             /* offset of the clique's true observations in `obs`                 */
    int32_t sep_off;             /* offset in `cols` of the n_sep source column indices               */
    int32_t front_off;           /* offset in `cols` of the n_frontal destination column indices      */
    int32_t reserved;
} nfisam_post_clique;

/* FactorGraphSolver.sample_posterior (src/slam/FactorGraphSolver.py:497-550) for a whole tree in ONE
 * launch: for every clique in `table` order (root first) sample its frontal columns conditioned on its
 * true observations and on the separator columns sampled earlier, exactly as n_cliques successive
 * conditional_sample_given_observation calls would (slam/NFiSAM.py:120-155), but without leaving
 * the device.  Zt[total_dim][n]: standard-normal draws, consumed in WALK order (the j-th frontal column of
 * clique c takes row sum_{c'<c} n_frontal(c') + j), St[total_dim][n]: output samples (rows = columns of `cols`), both
 * COLUMN-major; cols/obs: device arrays indexed by the table; max_D: largest D_model.        */
int nfisam_nsf_posterior_walk(const nfisam_post_clique* table, int n_cliques, const int32_t* cols, const float* obs,
                              int max_D, int K, int H, float B, int L, int n, const float* Zt, float* St,
                              nfisam_stream_t stream);

/* The joint log-density of the tree's posterior at n given points, not in the reference (whose per-sample
 * separator_forward / log_pdf is scrambled for n > 1): the walk run FORWARD.  For every clique c of
 * `table` (the walk's table, cols and obs, same meaning), with D = n_obs + n_sep + n_frontal:
 *   u = [true observations | separator columns | frontal columns] of the point, normalised as
 *       NormalizingFlowModelWithSeparator.normalize_samples (src/slam/NFiSAM.py:96-106: angle columns wrap(u - mean) / std
 *       with wrap to [-pi, pi), others (u - mean) / std);
 *   z = the L-layer forward of u (NSF_AR.forward, src/flows/flows.py:65-93; the first D of D_model dims, as
 *       NormalizingFlowModelWithSeparator.separator_forward evaluates a marginal, src/slam/NFiSAM.py:157-173);
 *   term_c = sum over the frontal columns d of [ -z_d^2/2 - log(2 pi)/2 + sum_l log|dz^l_d / dz^(l-1)_d| - log std_d ]
 *          = log q_c(frontal | separator, observations) in the variables' own units (metres, radians).
 * log_q[p] = sum of term_c over the cliques in table order.  Observation and separator columns only condition.  The density
 * is periodic in every angle; on the circle it is normalised up to the mass the flow puts beyond +-pi/std.
 *   St[total_dim][n]: the points, COLUMN-major as the walk writes them; log_q[n];
 *   per_clique[n_cliques][n] (nullable): term_c of every point -- without it the library takes a scratch buffer of that
 *     size from the stream-ordered allocator for the call;
 *   latent[total_dim][n] (nullable): z_d of every frontal column, at the row the walk reads that column's latent draw from
 *     (walk order: sum_{c' < c} n_frontal(c') + j); other rows are not written.
 * Two launches (one block per (clique, 64-point tile), then the per-point sum in table order); no float atomics: two calls
 * give the same bits.  The column indices in `cols` must lie in [0, total_dim) (the binding checks them; the device
 * table is not read on the host).  NFISAM_ERR_ARG: unsupported (K, H), NULL table / cols / St / log_q, a bad count. */
int nfisam_nsf_posterior_log_density(const nfisam_post_clique* table, int n_cliques, const int32_t* cols, const float* obs,
                                     int max_D, int K, int H, float B, int L, int n, const float* St, float* log_q,
                                     float* per_clique, float* latent, nfisam_stream_t stream);

/* Training-batch normalisation on the device (NFiSAM.normalize_training_samples, src/slam/NFiSAM.py:515-548):
 * per column c of x[n,D]: Euclidean -> mean / population std; circular[c] != 0 -> mean = direction of the mean
 * resultant (scipy.stats.circmean(., high=pi, low=-pi)), deviations wrapped to [-pi, pi), std of the wrapped
 * deviations; std clipped at 1e-5.  x_out[n,D] = (wrapped) deviation / std, mean[D], std[D].  Sums in double.
 * `circular` may be NULL (all Euclidean); x_out may alias x.                                             */
int nfisam_normalize_columns(const float* x, int n, int D, const uint8_t* circular, float* x_out, float* mean,
                             float* std, nfisam_stream_t stream);

/* ---- clique training-batch simulator (f-2) -------------------------------------------------------
 * One op of the ancestral-simulation schedule of a clique (sampler/SimulationBasedSampler.plan; reference:
 * src/sampler/SimulationBasedSampler.py:14-133).  Columns index the [n, D_total] batch; an SE(2) variable takes 3
 * consecutive columns (x y theta), an R2 variable 2.  p: SE(2) ops = pose / measurement (3) then the lower Cholesky
 * factor of the tangent-space noise covariance (l00 l10 l11 l20 l21 l22).                                     */
#define NFISAM_SIM_MAX_OPS 40
#define NFISAM_SIM_COPY       1   /* c.. <- k columns b.. of the row-major device array `src` with row stride a       */
#define NFISAM_SIM_PRIOR_SE2  2   /* c <- p[0:3] * Exp(eps)                       (Factors.py:725-743)                */
#define NFISAM_SIM_REL_FWD    3   /* c <- col a * (p[0:3] * Exp(eps))             (Factors.py:1196-1317)              */
#define NFISAM_SIM_REL_BWD    4   /* c <- col a * (p[0:3] * Exp(eps))^-1                                              */
#define NFISAM_SIM_REL_OBS    5   /* c <- (col a)^-1 (col b) * Exp(eps)           simulated odometry measurement      */
#define NFISAM_SIM_RING       6   /* c(xy) <- a(xy) + (p[0] + p[1] z)(cos phi, sin phi), phi ~ U(-pi, pi)  (:2575-2649) */
#define NFISAM_SIM_RANGE_OBS  7   /* c <- |b(xy) - a(xy)| + p[0] z                simulated range measurement         */
#define NFISAM_SIM_ADA_OBS    8   /* c <- range from a(xy) to ONE of the k candidates cand[], cumulative weights
                                     p[0:k], noise p[4] z                          (Factors.py:3146-3157)             */
#define NFISAM_SIM_NH_RING    9   /* RING whose noise is p[1] with probability p[3], else p[2]   (BinaryFactorWithNullHypo,   */
#define NFISAM_SIM_NH_OBS    10   /* RANGE_OBS whose noise is p[0] with probability p[2], else p[1]    Factors.py:3300-3462)  */
#define NFISAM_SIM_PRIOR_R2  11   /* c(xy) <- p[0:2] + L z, L = p[2] p[3] p[4] (l00 l10 l11)      (UnaryR2GaussianPriorFactor, :362)   */
#define NFISAM_SIM_PRIOR_R2_RING 12 /* c(xy) <- p[0:2] + (p[2] + p[3] z)(cos phi, sin phi)  (UnaryR2RangeGaussianPriorFactor, :451)      */
#define NFISAM_SIM_REL_R2_FWD 13  /* c(xy) <- a(xy) + p[0:2] + L z                                (R2RelativeGaussianLikelihoodFactor, */
#define NFISAM_SIM_REL_R2_BWD 14  /* c(xy) <- a(xy) - L z - p[0:2]                                 Factors.py:998-1030)                */
#define NFISAM_SIM_REL_R2_OBS 15  /* c(xy) <- b(xy) - a(xy) + L z                simulated displacement measurement                   */
typedef struct nfisam_sim_op {
    int32_t code;
    int32_t a, b, c;
    int32_t cand[4];
    int32_t k;
    float p[9];
    uint64_t src;
} nfisam_sim_op;

/* Simulate the n joint samples of a clique: every thread interprets `ops` (HOST array, copied into the launch) for its
 * own sample with a counter-based generator keyed by `seed`; x_out[n, D_out] row-major receives the first D_out
 * columns (D_total - D_out scratch columns may hold variables that are not part of the batch).
 * Generator: Philox4x32-10, counter (sample, op index, 0x9E3779B9, 0x243F6A88), key (seed low, seed high);
 * float32 uniforms on (0, 1]; z0 z1 from (u0, u1), z2 from (u2, u3), bearings and the ADA_OBS / NH_OBS picks from u2, the
 * NH_RING pick from u3.  NFISAM_ERR_ARG, before any launch: n_ops outside 1..NFISAM_SIM_MAX_OPS, D_total > 150, an op whose
 * a, b, cand[j < k] or c leaves the D_total columns, a COPY with b < 0 or b + k > a, k out of range.              */
int nfisam_simulate_clique(const nfisam_sim_op* ops, int n_ops, int n, int D_out, int D_total, uint64_t seed,
                           float* x_out, nfisam_stream_t stream);

/* ---- the factor graph's joint log-density ------------------------------------------------------------------
 * log p(X, Z) = sum over the factors f of log p_f(x_f) at n points, the reference's JointFactor.log_pdf
 * (src/sampler/sampler_utils.py:85-98) over its factors' `log_pdf` (src/factors/Factors.py).  One record per factor; a, b,
 * cand[] are FIRST ROWS of the variables in St (an SE(2) variable takes 3 consecutive rows x y theta, an R2 variable 2; range
 * codes read the first two rows of either kind).  p[] by code -- Gaussians carry the upper triangle of the precision matrix
 * (row-major: 6 entries for 3x3, 3 for 2x2) and their log normaliser -(d log 2 pi + log det Sigma) / 2:              */
#define NFISAM_FAC_PRIOR_SE2      1 /* N(Log(p[0:3]^-1 * a); 0, Sigma) + log|det dLog|; p[3:9] precision, p[9] log norm
                                       (UnarySE2ApproximateGaussianPriorFactor, Factors.py:823-827; Log and its Jacobian
                                       det = th^2 / (4 sin^2(th/2)), 1 for |th| < 1e-5: geometry/TwoDimension.py:405-441)  */
#define NFISAM_FAC_REL_SE2        2 /* the same of p[0:3]^-1 * (a^-1 * b)  (SE2RelativeGaussianLikelihoodFactor, :1443-1448)   */
#define NFISAM_FAC_RANGE          3 /* N(|a_xy - b_xy| - p[0]; 0, 1 / p[1]), p[2] log norm  (SE2R2RangeGaussianLikelihoodFactor
                                       :2724-2730, R2RangeGaussianLikelihoodFactor :2195-2201)                          */
#define NFISAM_FAC_RANGE_MIX      4 /* log sum_{j<k} exp(range term of (a, cand[j]) with p[3j] measurement, p[3j+1] 1 / sigma^2,
                                       p[3j+2] log norm + log weight), by log-sum-exp  (BinaryFactorMixture, :3126-3133:
                                       AmbiguousDataAssociationFactor; BinaryFactorWithNullHypo = k 2, one landmark twice
                                       with two sigmas)                                                                 */
#define NFISAM_FAC_PRIOR_R2       5 /* N(a - p[0:2]; 0, Sigma); p[2:5] precision, p[5] log norm  (UnaryR2GaussianPriorFactor, :373)  */
#define NFISAM_FAC_PRIOR_R2_RANGE 6 /* N(|a - p[0:2]| - p[2]; 0, 1 / p[3]), p[4] log norm  (UnaryR2RangeGaussianPriorFactor, :2226:
                                       the range term :2195-2201 with one end at the centre)                            */
#define NFISAM_FAC_REL_R2         7 /* N(b - a - p[0:2]; 0, Sigma); p[2:5] precision, p[5] log norm
                                       (R2RelativeGaussianLikelihoodFactor, :1070-1074)                                 */
typedef struct nfisam_factor_term {
    int32_t code;
    int32_t a, b;          /* first rows of the factor's variables (b unused by unary factors and mixtures) */
    int32_t k;             /* mixture components, 1..4 (RANGE_MIX only) */
    int32_t cand[4];       /* first rows of the candidate landmarks */
    double p[16];
} nfisam_factor_term;

/* log_p[p] = sum_f term_f(point p), float64, for the n points of St[total_dim][n] -- the COLUMN-major float32 sample matrix
 * the tree walk writes and nfisam_nsf_posterior_log_density reads.  Float32 points in, float64 arithmetic, float64 out: the
 * value of the float64 formula at the float32 point (heading wraps are theta_to_pipi, utils/Functions.py:20-21).
 *   terms[n_terms]: DEVICE array;  per_factor[n_terms][n] (nullable): every term -- without it the library takes a scratch
 *   buffer of that size from the stream-ordered allocator for the call.
 * Two launches: one wave per (64-point tile, run of 8 factors) writes the terms, then one thread per point adds them
 * strictly in table order: log_p[p] == ((term_0 + term_1) + term_2) + ... in float64, independent of n and of the tile.  No
 * float atomics: two calls give the same bits.
 * NFISAM_ERR_ARG: NULL terms / St / log_p, a negative count, total_dim < 1, more than 524280 factors.  The library does not
 * read the device table on the host: a record with an unknown code, k outside 1..4 or a row outside [0, total_dim) yields NaN
 * for its term (nothing is read out of bounds); the Python binding refuses such tables before upload.               */
int nfisam_factor_graph_log_density(const nfisam_factor_term* terms, int n_terms, const float* St, int total_dim, int n,
                                    double* log_p, double* per_factor, nfisam_stream_t stream);

/* ---- the score of the joint density (factor_score.hip) -----------------------------------------------------------------
 * Gt[r][p] = d/dx_r log p(X, Z) at point p: the reference's JointFactor.grad_x_log_pdf (src/sampler/sampler_utils.py:100-113)
 * over its factors' `grad_x_log_pdf` (src/factors/Factors.py:829-850, :1450-1478, :2203-2223, :2732-2751, :3135-3156), for the
 * table and the sample matrix of nfisam_factor_graph_log_density.  Float32 points in, float64 arithmetic, float64 out: the
 * derivative of the float64 formula of the value entry at the float32 point -- of the smooth formula everywhere (small-angle
 * series of the log map and of its Jacobian below |w| = 0.2; the value's |w| < 1e-10 / 1e-5 branches get no plateaus), the
 * zero vector at a range of exactly 0, softmax weights with the value's max shift for mixtures (finite far from every
 * component).
 *   Factor f owns the slots slot_off[f] .. + {3, 6, 4, 2 + 2k, 2, 2, 4}[code] of scratch[n_slots][n], one per row it touches,
 *   in the order a's rows, then b's or the candidates'; row r of Gt is the sum of the slots row_slot[row_off[r] ..
 *   row_off[r + 1]), strictly in that order (the host lists a row's slots in table order); a row without a slot is 0.
 *   terms[n_terms], slot_off[n_terms], row_off[total_dim + 1], row_slot[n_slots]: DEVICE arrays; Gt[total_dim][n] double;
 *   scratch: nfisam_factor_graph_score_scratch_count(n_slots, n) doubles on the device.
 * Two launches, no float atomics: two calls give the same bits, and a point's column does not depend on n or on its tile.
 * NFISAM_ERR_ARG: a NULL pointer, a negative count, total_dim < 1 or > 65535, more than 524280 factors, n_slots > 10 n_terms.
 * The device tables are not read on the host: a record with an unknown code, k outside 1..4 or a row outside [0, total_dim)
 * yields NaN in its slots, a slot index or list outside the scratch yields NaN for its row (nothing is read or written out of
 * bounds); the Python binding refuses such tables before upload.  (Additive: ABI 1600.)                               */
size_t nfisam_factor_graph_score_scratch_count(int n_slots, int n);
int nfisam_factor_graph_score(const nfisam_factor_term* terms, int n_terms, const float* St, int total_dim, int n,
                              const int32_t* slot_off, int n_slots, const int32_t* row_off, const int32_t* row_slot, double* Gt,
                              double* scratch, nfisam_stream_t stream);

/* ---- Hessian-vector products of the joint density (factor_hessian.hip) -----------------------------------------------------
 * Ht[r][p] = sum_c d^2 log p / dx_r dx_c (X_p) * Vt[c][p]: the derivative of the score entry's smooth float64 formula along the
 * direction Vt, at the float32 point (not in the reference; matrix-free Newton steps and Laplace covariances need nothing
 * denser).  Small-angle series of a''(w) and l''(w) below |w| = 0.6; the zero vector at a range of exactly 0, like the score;
 * mixtures: sum_j r_j (H_j v + g_j (g_j . v)) - g (g . v) with the score's softmax weights (finite far from every component).
 *   The table, St, slot_off / n_slots / row_off / row_slot: those of nfisam_factor_graph_score, unchanged (a factor's share of
 *   H v is one number per row it touches: the same slots, the same ordered gather).  Vt[total_dim][n], Ht[total_dim][n] double;
 *   Gt[total_dim][n] double or NULL: with Gt the same first pass also evaluates the score's slots, and Gt is
 *   nfisam_factor_graph_score's result BIT FOR BIT (a Newton step needs g and H v at one point); Ht is the same bits with and
 *   without Gt.  scratch: nfisam_factor_graph_hvp_scratch_count(n_slots, n, Gt != NULL) doubles on the device.
 * Two launches (three with Gt), no float atomics: two calls give the same bits, and a point's column does not depend on n or
 * on its tile.  n == 0: nothing is done; n_terms == 0: a zero Ht (and Gt).
 * NFISAM_ERR_ARG: the score entry's refusals, and a NULL Vt.  A bad record reads nothing of St or Vt and yields NaN in its
 * slots, as there.  (Additive: ABI 1600.)                                                                              */
size_t nfisam_factor_graph_hvp_scratch_count(int n_slots, int n, int with_score);
int nfisam_factor_graph_hvp(const nfisam_factor_term* terms, int n_terms, const float* St, const double* Vt, int total_dim, int n,
                            const int32_t* slot_off, int n_slots, const int32_t* row_off, const int32_t* row_slot, double* Ht,
                            double* Gt, double* scratch, nfisam_stream_t stream);

/* ---- two-sample MMD: the kernel sums of many column blocks in one launch (sample_mmd.hip) ---------------------------------
 * The reference grades a posterior against a reference sample set with an RBF-kernel MMD (src/utils/Statistics.py:13-84).
 * Block b of the table compares the entries col_off .. col_off + d of the row lists: entry e pairs row xcols[e] of Xt with
 * row ycols[e] of Yt (the reference set has its own variable order).  Blocks may overlap and repeat entries. */
typedef struct nfisam_mmd_block {
    int32_t col_off;           /* first entry of the block in xcols / ycols / scale / wrap */
    int32_t d;                 /* number of entries, >= 1 (no upper limit) */
    double inv_two_sigma2;     /* 1 / (2 sigma^2) of the block's kernel, positive and finite */
} nfisam_mmd_block;

/* sums[b] = { Sxx, Syy, Sxy } (double[n_blocks][3]): the sums of k_b over ALL ordered pairs of the m columns of Xt, of the n
 * columns of Yt, and of one of each (a pair i = i contributes exactly 1), with
 *     k_b(u, v) = exp(-inv_two_sigma2 * sum_e diff_e^2),  diff_e = (double)u_e - (double)v_e,
 * then wrapped into [-pi, pi) where wrap[e] is set (the sign convention of theta_to_pipi), then multiplied by scale[e].
 *   Xt[x_rows][m], Yt[y_rows][n]: COLUMN-major float32 device matrices (the layout of the tree walk's St);
 *   blocks[n_blocks]: HOST copy of the table (validated here), blocks_dev: DEVICE copy of the same table (what the kernel reads);
 *   xcols, ycols [n_entries] int32, scale [n_entries] double (nullable), wrap [n_entries] uint8 (nullable): DEVICE arrays;
 *   scratch: nfisam_sample_mmd_scratch_count(m, n, n_blocks) doubles on the device (per-tile partials).
 * Float32 points in; float64 differences, squared distance, exp and sums.  Two launches, no float atomics: a 256-thread
 * group per (64 x 64 tile of pairs, block, sum) writes one partial, then a wave per (block, sum) adds the partials in an order
 * that depends on (m, n) alone: two calls give the same bits, and a block's sums are the same bits alone or among hundreds,
 * wherever it stands in the table.
 * NFISAM_ERR_ARG: a NULL pointer (scale and wrap excepted), m, n, x_rows, y_rows, n_entries or n_blocks < 1, a block with
 * d < 1 or inv_two_sigma2 not positive and finite, more than 65535 blocks or more than 2^31 - 1 tiles.  The device arrays are
 * not read on the host: a block whose entries leave [0, n_entries) or that names a row outside its matrix yields NaN for its
 * three sums (nothing is read out of bounds); the Python binding refuses such tables before upload.  (Additive: ABI 1600.) */
size_t nfisam_sample_mmd_scratch_count(int m, int n, int n_blocks);     /* 0 for arguments the entry refuses */
int nfisam_sample_mmd(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n, const nfisam_mmd_block* blocks,
                      const nfisam_mmd_block* blocks_dev, int n_blocks, const int32_t* xcols, const int32_t* ycols, int n_entries,
                      const double* scale, const uint8_t* wrap, double* sums, double* scratch, nfisam_stream_t stream);

/* ---- the MMD permutation test: the kernel sums under many relabellings of the pooled set (sample_mmd_perm.hip) -------------
 * What the number nfisam_sample_mmd gives is worth: pool the two sets, relabel them n_perms times and ask how often the
 * relabelled MMD reaches the observed one.  Pooled point q is column q of Xt for q < m and column q - m of Yt otherwise; with K
 * the block's kernel on the pooled set (formula, wrap and scale word for word those of nfisam_sample_mmd), l in {0,1}^(m + n)
 * a relabelling with m ones, t = K 1 and T = 1' K 1,
 *     sums[b][p] = { Sxx', Syy', Sxy' } = { l' K l,  T - 2 l' t + l' K l,  l' t - l' K l }      (double[n_blocks][n_perms][3]):
 * the three sums of nfisam_sample_mmd between the points labelled 1 and the points labelled 0, ready for the same estimators.
 *   labels: DEVICE, [m + n][W] uint64, W = (n_perms + 63) / 64: bit p & 63 of word [q][p >> 6] is set when pooled point q
 *   counts as the first set under permutation p; bits past n_perms are ignored.  The entry does not read device data on the
 *   host: that every permutation has exactly m set bits is the caller's check (the Python binding makes it).
 *   n_perms: 1 .. NFISAM_MMD_PERM_MAX a call (callers split longer lists: a permutation's numbers do not depend on the split);
 *   scratch: nfisam_sample_mmd_perm_scratch_count doubles on the device: two per (block, strip of 64 pooled points,
 *   permutation rounded up to 256) and one per (block, strip); every other argument as in nfisam_sample_mmd.
 * Every Gram value is evaluated once per 256 permutations, then costs one float64 multiply-add (v_mfma_f64_16x16x4_f64) per
 * permutation.  Two launches, no float atomics: a 256-thread group per (tile row of the pooled upper triangle, block, 256
 * permutations), then a thread per (block, permutation) adds the strips in an order that depends on (m, n) alone: two calls
 * give the same bits; a block's numbers are the same bits alone or anywhere in a table; a permutation's numbers are the same
 * bits alone, first or last of a call.
 * NFISAM_ERR_ARG, before any launch: what nfisam_sample_mmd refuses, a NULL labels, n_perms outside 1 .. NFISAM_MMD_PERM_MAX,
 * more than 2^24 - 1 groups (strips x chunks of 256 permutations x blocks).  Bad table entries or rows yield NaN for that
 * block and nothing is read out of bounds, as there.  (Additive: ABI 1600.) */
#define NFISAM_MMD_PERM_MAX 16384
size_t nfisam_sample_mmd_perm_scratch_count(int m, int n, int n_blocks, int n_perms);   /* 0 for arguments the entry refuses */
int nfisam_sample_mmd_perm(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n,
                           const nfisam_mmd_block* blocks, const nfisam_mmd_block* blocks_dev, int n_blocks,
                           const int32_t* xcols, const int32_t* ycols, int n_entries, const double* scale, const uint8_t* wrap,
                           const uint64_t* labels, int n_perms, double* sums, double* scratch, nfisam_stream_t stream);

/* ---- sliced Wasserstein: every (block, direction) slice of two sample sets in one launch (sample_transport.hip) --------------
 * Not in the reference (its src/utils/Statistics.py stops at MMD, RMSE and KSD): how far, in the variables' own units, one
 * sample set must be moved to become the other.  Block b of the table holds the entries col_off .. col_off + d of the row
 * lists (entry e pairs row xcols[e] of Xt with row ycols[e] of Yt, as in nfisam_sample_mmd) and n_dirs directions of d doubles
 * each, direction j at dirs[dir_off + j d ..]; its slices are out[out_off .. out_off + n_dirs).  Blocks may overlap and
 * repeat entries; their directions and results are their own. */
typedef struct nfisam_transport_block {
    int32_t col_off;           /* first entry of the block in xcols / ycols / kind / scale */
    int32_t d;                 /* number of entries, >= 1 (no upper limit) */
    int32_t n_dirs;            /* number of directions, 1 .. 65535 */
    int32_t reserved;          /* 0 */
    int64_t dir_off;           /* first double of the block's directions in dirs: [n_dirs][d] */
    int64_t out_off;           /* the block's first slice in out */
} nfisam_transport_block;

#define NFISAM_TRANSPORT_MAX_N 8192  /* most points per set: two lists of float64 keys in LDS, 128 KiB */
/* out[out_off_b + j] = W_p^p of the two sets projected on direction j of block b, with
 *     key(x) = sum_e dir[j][e] * scale[e] * f_e((double)x_e)  in ascending e,  f_e by kind[e]: 0 the value, 1 cos, 2 sin,
 *     W_p^p  = int_0^1 |F_X^-1(t) - F_Y^-1(t)|^p dt = sum_i sum_j w_ij |a_i - b_j|^p / (m n)  on the sorted keys a [m], b [n],
 *     j = floor(i n / m) .. ceil((i + 1) n / m) - 1,  w_ij = min((i + 1) n, (j + 1) m) - max(i n, j m):
 * for m == n the mean of |a_(i) - b_(i)|^p, by the same loop.  A heading enters a block as two entries naming the same row, one
 * cos and one sin (the chord embedding: continuous across +-pi, the radian difference for small differences); there is no
 * wrap flag.  A basis vector as direction gives the exact 1-D W_p^p of that entry's marginal.
 *   Xt[x_rows][m], Yt[y_rows][n]: COLUMN-major float32 device matrices (the layout of the tree walk's St);
 *   blocks[n_blocks]: HOST copy of the table (validated here), blocks_dev: DEVICE copy of the same table (what the kernel reads);
 *   xcols, ycols [n_entries] int32, kind [n_entries] uint8 (nullable: all 0), scale [n_entries] double (nullable: all 1),
 *   dirs [dirs_count] double, out [out_count] double: DEVICE arrays;  p: 1 or 2.
 * Float32 points in; float64 projection, cos / sin, keys and sums.  One launch, no float atomics: a 256-thread group per
 * (direction, block) projects both sets, sorts both key lists in 8 (pad(m) + pad(n)) bytes of dynamic LDS (bitonic, padded
 * with +inf to powers of two) and adds the pieces in a fixed order: two calls give the same bits; a block's slices are the
 * same bits alone, repeated or anywhere in a table; a direction's slice is the same bits alone or among others.  A slice
 * with a non-finite key is NaN.
 * NFISAM_ERR_ARG, before any launch: a NULL pointer (kind and scale excepted), m, n, x_rows, y_rows, n_entries or n_blocks < 1,
 * m or n > NFISAM_TRANSPORT_MAX_N, p not 1 or 2, more than 65535 blocks, a block with d < 1 or n_dirs outside 1 .. 65535, a
 * block whose directions leave [0, dirs_count) or whose slices leave [0, out_count).  The device arrays are not read on the
 * host: a block whose entries leave [0, n_entries), that names a row outside its matrix or that has a kind > 2 yields NaN
 * in all its slices, reads nothing out of bounds and leaves every other block untouched; the Python binding refuses such
 * tables before upload.  (Additive: ABI 1600.) */
int nfisam_sample_sliced_transport(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n,
                                   const nfisam_transport_block* blocks, const nfisam_transport_block* blocks_dev, int n_blocks,
                                   const int32_t* xcols, const int32_t* ycols, const uint8_t* kind, const double* scale,
                                   int n_entries, const double* dirs, long long dirs_count, int p, double* out,
                                   long long out_count, nfisam_stream_t stream);

/* ---- kernel Stein discrepancy: the pairwise Stein sums of a sample set and its scores (sample_ksd.hip) -----------------------
 * The reference's Gaussian_kernel_stein_discrepancy (src/utils/Statistics.py:216-245) for a DIAGONAL kernel precision p[rows],
 * p_c >= 0.  With d = x_i - x_j, brought into [-pi, pi] as sign(d) wrap(|d|) where wrap[c] is set, and s = the scores:
 *     k_ij = exp(-1/2 sum_c p_c d_c^2),   h_ij = k_ij [ s_i.s_j + sum_c (s_ic - s_jc) p_c d_c - sum_c p_c^2 d_c^2 + sum_c p_c ]
 *     row[i] = sum over ALL j of h_ij,  diag[i] = h_ii = |s_i|^2 + sum_c p_c,  H[i][j] = h_ij (nullable; n <= 4096: 128 MiB).
 *   Xt[rows][n]: COLUMN-major float32 device matrix; Gt[rows][n]: COLUMN-major float64 device matrix (what
 *   nfisam_factor_graph_score writes); precision[rows] double, wrap[rows] uint8 (nullable): DEVICE arrays;
 *   row[n], diag[n], H[n][n] double; scratch: nfisam_sample_ksd_scratch_count(n) doubles on the device.
 * Float32 points in; float64 differences, products, exp and sums; direct differences.  Two launches, no float atomics: a
 * 256-thread group per 64 x 64 tile of the full grid of pairs writes one partial per (tile, i), then row[i] adds them in tile
 * order: two calls give the same bits, `row` is the same bits with and without H, and H is symmetric to the bit.
 * NFISAM_ERR_ARG: a NULL pointer (wrap and H excepted), rows or n < 1, n > 65535 * 64, H with n > 4096.  The precision is not
 * read on the host: the Python binding refuses negative or non-finite entries before upload.  (Additive: ABI 1600.)   */
#define NFISAM_KSD_MATRIX_MAX_N 4096
size_t nfisam_sample_ksd_scratch_count(int n);                          /* 0 for an n the entry refuses */
int nfisam_sample_ksd(const float* Xt, const double* Gt, int rows, int n, const double* precision, const uint8_t* wrap,
                      double* row, double* diag, double* H, double* scratch, nfisam_stream_t stream);

/* ---- Stein variational direction and step: posterior samples moved along the joint score (sample_svgd.hip) --------------------
 * phi(x_i) = 1/n sum_j [ k(x_j, x_i) grad log p(x_j) + grad_{x_j} k(x_j, x_i) ] (Liu & Wang 2016; not in the reference), per
 * block of the nfisam_mmd_block table: block b owns the entries col_off .. col_off + d of `cols`, entry e names row cols[e] of Xt
 * and of Gt, and its kernel sees the block's own columns only.  With d_ij,e = x_i - x_j in row cols[e], brought into [-pi, pi] as
 * sign(d) wrap(|d|) where wrap[e] is set (d_ji = -d_ij to the bit):
 *     k_b(i, j) = exp(-inv_two_sigma2 sum_e (scale_e d_ij,e)^2)
 *     phi[e][i] = ( sum_j k_b(i, j) ( Gt[cols[e]][j] + 2 inv_two_sigma2 scale_e^2 d_ij,e ) ) / n
 * An entry with scale_e = 0 leaves the kernel and still gets its sum_j k g / n; d has no upper limit.
 *   Xt[x_rows][n]: COLUMN-major float32 device matrix; Gt[x_rows][n]: COLUMN-major float64 device matrix (what
 *   nfisam_factor_graph_score writes); blocks[n_blocks]: HOST copy of the table (validated here), blocks_dev: DEVICE copy (what
 *   the kernels read); cols [n_entries] int32, scale [n_entries] double (nullable: 1), wrap [n_entries] uint8 (nullable): DEVICE
 *   arrays; phi[n_entries][n] double, ENTRY-major: blocks own disjoint entries, so no two blocks write one address; an entry
 *   that no block owns is left as it was; scratch: nfisam_sample_svgd_scratch_count(n, n_blocks, n_entries) doubles on the device.
 * Float32 points in; float64 differences, products, exp and sums; direct differences.  Two launches, no float atomics: a
 * 256-thread group per (64 x 64 tile of pairs, block) walks the block's columns twice in chunks of 16 -- the squared distances and
 * the 64 x 64 kernel values, then per column the sums over the tile's j -- and writes one partial per (tile of j, entry, i); then
 * phi[e][i] adds them in tile order and divides by n.  Two calls give the same bits, and a block's rows are the same bits alone or
 * among hundreds, wherever it stands in the table; swapping the two points of a two-point set swaps their phi bit for bit.
 * NFISAM_ERR_ARG: a NULL pointer (scale and wrap excepted), x_rows, n, n_entries or n_blocks < 1, a block with d < 1 or
 * inv_two_sigma2 not positive and finite, two blocks that share an entry, more than 65535 blocks, n > 65535 * 64.  The device
 * arrays are not read on the host: a block whose entries leave [0, n_entries) or that names a row outside the matrix yields NaN
 * for its entries (nothing is read or written out of bounds); the Python binding refuses such tables before upload.
 *
 * nfisam_sample_step applies phi to the points in place, the AdaGrad-with-decay rule of the original SVGD code, in float64 per
 * (entry e, point i):
 *     hist = first ? phi^2 : alpha hist + (1 - alpha) phi^2
 *     y    = (double)Xt[cols[e]][i] + eps[e] phi / (sqrt(hist) + fudge)
 *     Xt[cols[e]][i] = (float)(wrap[e] ? wrap_pi(y) : y)          (wrap_pi: into [-pi, pi), the sign convention of theta_to_pipi)
 *   eps[n_entries] double: DEVICE array, one step length per entry in the column's own unit; hist[n_entries][n] double: the
 *   caller's state, read unless `first`, always written; phi as nfisam_sample_svgd writes it (or any direction of that layout).
 * The points stay float32: a step smaller than the float32 spacing of a coordinate is lost (7.6e-6 at 100 m).  A wrapped value
 * that rounds to +-float32(pi), outside [-pi, pi), becomes the float32 just inside -pi.  One launch, elementwise: the same bits
 * on every call.  A row of Xt named by two entries would be written twice: the Python binding refuses it.
 * NFISAM_ERR_ARG: a NULL pointer (wrap excepted), x_rows, n or n_entries < 1, n_entries > 65535, alpha outside [0, 1), fudge not
 * positive and finite.  An entry whose row lies outside the matrix moves nothing and gets NaN in hist.  (Additive: ABI 1600.) */
size_t nfisam_sample_svgd_scratch_count(int n, int n_blocks, int n_entries);   /* 0 for arguments the entry refuses */
int nfisam_sample_svgd(const float* Xt, int x_rows, int n, const double* Gt, const nfisam_mmd_block* blocks,
                       const nfisam_mmd_block* blocks_dev, int n_blocks, const int32_t* cols, int n_entries, const double* scale,
                       const uint8_t* wrap, double* phi, double* scratch, nfisam_stream_t stream);
int nfisam_sample_step(float* Xt, int x_rows, int n, const int32_t* cols, int n_entries, const uint8_t* wrap, const double* phi,
                       double* hist, const double* eps, double alpha, double fudge, int first, nfisam_stream_t stream);

/* ---- Metropolis-corrected moves: the Langevin / random-walk proposal and the accept step of n chains (sample_mcmc.hip) --------
 * Not in the reference.  A chain is a column of Xt; h[x_rows] double >= 0 is the step length of a row in its own unit (0 freezes
 * the row), wrap[x_rows] uint8 (nullable) marks angles: DEVICE arrays.  Xt, Yt [x_rows][n]: COLUMN-major float32 device
 * matrices; Gx, Gy [x_rows][n]: COLUMN-major float64 (what nfisam_factor_graph_score writes).  All arithmetic float64.
 *
 * THE GENERATOR (a contract: DESIGN.md 3.3k): Philox4x32-10, the constants of nfisam_simulate_clique; key (seed & 0xffffffff,
 * seed >> 32); counter (chain i, row r >> 2, step t, tag), tag 0 the normals, tag 1 the accept uniform with row word 0;
 * u = (word + 0.5) 2^-32 in float64, inside (0, 1) exactly; the four normals of a counter block are Box-Muller (cos, sin) of
 * (u0, u1) -> rows 4g, 4g + 1 and of (u2, u3) -> rows 4g + 2, 4g + 3.  A chain's draws depend on (seed, i, r, t) alone.
 *
 * nfisam_sample_propose:  Yt[r][i] = x + (h_r^2 / 2) Gx[r][i] + h_r z  (Gx NULL: the random walk x + h_r z), wrapped into
 * [-pi, pi) where wrap[r] is set and rounded to float32 by nfisam_sample_step's rule (a wrapped value that rounds to
 * +-float32(pi) becomes the float32 just inside -pi).  A row with h_r == 0 is copied bit for bit.  Xt is not written.  One
 * launch, elementwise: the same bits on every call, at any n.
 * NFISAM_ERR_ARG: a NULL pointer (Gx and wrap excepted), x_rows or n < 1, n > 65535 * 64, x_rows > 65535 * 32.
 *
 * nfisam_sample_accept:  per chain i, with d_r = (double)Xt[r][i] - (double)Yt[r][i] -- the values actually stored, so the ratio
 * is exact for the move that was made -- brought into [-pi, pi] as sign(d) wrap(|d|) where wrap[r] is set (the nearest image of
 * the wrapped normal; the caller bounds h on such rows), and a_r = h_r^2 / 2:
 *     log_alpha[i] = (lp_y[i] - lp_x[i]) + sum_{r: h_r > 0} [ 1/2 ((-d_r - a_r Gx[r][i]) / h_r)^2 - 1/2 ((d_r - a_r Gy[r][i]) / h_r)^2 ]
 * (Gx and Gy both NULL: no sum, a symmetric proposal -- the random walk, or an independence step with lp = log p - log q).
 * accepted[i] = log(u) < log_alpha[i]: a NaN log_alpha rejects, lp_y = -inf rejects, lp_x = -inf with a finite lp_y accepts.  On
 * accept column i of Yt replaces column i of Xt, column i of Gy that of Gx and lp_y[i] replaces lp_x[i]; a rejected chain keeps
 * every bit.  Two launches, no float atomics: the row sum is taken in an order that depends on x_rows alone (a thread's rows
 * ascending, the four waves in order, slabs of 32 rows in slab order through `scratch`), so log_alpha[i] is the same bits on
 * every call, at any n and in any tile.  scratch: nfisam_sample_accept_scratch_count(x_rows, n) doubles on the device.
 * NFISAM_ERR_ARG: a NULL pointer (Gx and Gy together, and wrap, excepted), Gx without Gy or the reverse, x_rows or n < 1,
 * n > 65535 * 64, x_rows > 65535 * 32.  h is not read on the host: the Python binding refuses negative or non-finite entries
 * before upload.  (Additive: ABI 1600.) */
int nfisam_sample_propose(const float* Xt, const double* Gx, float* Yt, int x_rows, int n, const double* h, const uint8_t* wrap,
                          uint64_t seed, uint32_t t, nfisam_stream_t stream);
size_t nfisam_sample_accept_scratch_count(int x_rows, int n);           /* 0 for arguments the entry refuses */
int nfisam_sample_accept(float* Xt, const float* Yt, double* Gx, const double* Gy, double* lp_x, const double* lp_y, int x_rows,
                         int n, const double* h, const uint8_t* wrap, uint64_t seed, uint32_t t, double* log_alpha,
                         uint8_t* accepted, double* scratch, nfisam_stream_t stream);

/* ---- chain diagnostics: split-R-hat, the blocking autocorrelation time and the within-chain variance per row (sample_chains.hip)
 * Not in the reference.  The n chains are the columns of Xt[x_rows][n] (COLUMN-major float32, device); their history is never
 * kept: one nfisam_chain_record per recorded state t = 0 ... T - 1, ASCENDING, folds it into `state`, and nfisam_chain_finish
 * turns the state into per-row statistics.  T is even and >= 2; levels (the blocking levels, level 0 included) lies in
 * [1, min(NFISAM_CHAIN_MAX_LEVELS, floor(log2 T))], so every level has at least two blocks.  center[x_rows] double (NULL: 0) and
 * wrap[x_rows] uint8 (NULL: no angles) are DEVICE arrays, the same in every call of a run.  All arithmetic float64.
 *
 * The recorded value of row r, chain i:  v = (double)Xt[r][i] - center[r], wrapped into [-pi, pi) where wrap[r] is set.
 * state: nfisam_chain_state_count(x_rows, n, levels) = (4 + 3 (levels - 1)) x_rows n doubles, slot-major [slot][row][chain], ZEROS
 * before t = 0:  slots 0, 1: A1[w] = sum v;  slots 2, 3: A2[w] = sum v^2, w = 0 for t < T / 2 and 1 for t >= T / 2;  slots
 * 4 + 3 (l - 1) + {0, 1, 2}: P_l, R_l, Q_l of level l = 1 ... levels - 1 (Flyvbjerg & Petersen 1989): the pending value, and the sums
 * R_l = sum_j b_lj, Q_l = sum_j b_lj^2 over the means b_lj of the complete blocks of 2^l consecutive values.  Level 0 is the
 * halves added up.
 *
 * nfisam_chain_record, the fold at index t:  A1[w] += v, A2[w] += v^2; carry = v; for l = 1 ... levels - 1: bit l - 1 of t clear
 * -> P_l = carry, stop; set -> carry = (P_l + carry) / 2, R_l += carry, Q_l += carry^2, go on.  Xt is not written.  One launch,
 * elementwise: the same bits on every call, at any n, for a row alone or inside a taller matrix.
 * NFISAM_ERR_ARG before any launch: Xt or state NULL, x_rows or n < 1, n > 65535 * 64, T odd or < 2, t >= T, levels out of range.
 *
 * nfisam_chain_finish, per row over its n chains, with m_l = T >> l and s2_li = (Q_l - R_l^2 / m_l) / (m_l - 1):
 *     mean[r]   = center[r] + sum_i (A1[0] + A1[1]) / (n T), wrapped where wrap[r] is set
 *     within[r] = mean_i s2_0i                               the pooled within-chain variance of whole chains
 *     tau[l][r] = 2^l mean_i s2_li / mean_i s2_0i            the blocking estimate of the integrated autocorrelation time at
 *                                                            block length 2^l; tau[0] = 1 by construction
 *     rhat[r]   = sqrt(((L - 1) / L W + B / L) / W)          split-R-hat (BDA3 11.4) over the 2 n half-chains of length L = T / 2:
 *                 mu_k = A1 / L, s2_k = (A2 - A1^2 / L) / (L - 1), W = mean_k s2_k, B / L = sum_k (mu_k - mu_bar)^2 / (2 n - 1) with
 *                 mu_bar taken first (two passes).  NaN for T < 4, and NaN where W = 0 and B = 0 (a row without spread): 0 / 0, no
 *                 special case.  (A row frozen at a different constant per chain has W = 0 only up to the rounding of its sums:
 *                 the caller, who knows which rows are frozen, discards their rhat and tau.)
 * mean, within, rhat [x_rows] and tau [levels][x_rows]: double, device.  One block per row, no float atomics: a thread adds its
 * chains ascending, then the fixed wave tree, then the four waves in order -- the same bits on every call, for a row alone
 * or inside a taller matrix.
 * NFISAM_ERR_ARG before any launch: state or a result NULL, x_rows or n < 1, n > 65535 * 64, T odd or < 2, levels out of range.
 * (Additive: ABI 1600.) */
#define NFISAM_CHAIN_MAX_LEVELS 16
size_t nfisam_chain_state_count(int x_rows, int n, int levels);         /* 0 for arguments the entries refuse */
int nfisam_chain_record(const float* Xt, double* state, int x_rows, int n, int levels, const double* center, const uint8_t* wrap,
                        uint32_t t, uint32_t T, nfisam_stream_t stream);
int nfisam_chain_finish(const double* state, int x_rows, int n, int levels, uint32_t T, const double* center, const uint8_t* wrap,
                        double* mean, double* within, double* rhat, double* tau /* [levels][x_rows] */, nfisam_stream_t stream);

/* ---- sample summaries: means, resultant lengths, covariances and quantiles of many column blocks (sample_summary.hip) -------
 * The reference summarises a draw on the host: `sample_mean` (src/utils/Statistics.py:151-171: np.mean, and scipy's
 * circmean(high = pi, low = -pi) for headings) and, built on it, `rmse` (:142-148), `geodesic_distance` (:179-191) and
 * `translation_distance` (:204-214).  Here the COLUMN-major float32 device matrix Xt[x_rows][n] (the tree walk's St, the layout
 * of nfisam_sample_mmd) is summarised where it lies.  Entry e names the row cols[e] of Xt; block b of the table is the run of
 * entries col_off .. col_off + d.  Rows may repeat within a block and between blocks.
 * Float32 points in; every difference, product, transcendental and sum is float64.  No float atomics: an entry's and a block's
 * results are the same bits alone, repeated, anywhere in a table, and on a second call. */
#define NFISAM_MOMENTS_MAX_D  16     /* widest block: a pose is 3, a pose and a landmark 5, two poses 6 */
#define NFISAM_QUANTILE_MAX_N 16384  /* most points per column the quantile sort takes: 128 KiB of float64 keys in LDS */
typedef struct nfisam_moment_block {
    int32_t col_off;           /* first entry of the block in cols / circular / mean / resultant */
    int32_t d;                 /* number of entries, 1 .. NFISAM_MOMENTS_MAX_D */
    int64_t cov_off;           /* where the block's d x d row-major matrix starts in cov */
} nfisam_moment_block;

/* nfisam_sample_moments replaces Statistics.py:151-171 (and the per-variable np.cov of the run scripts).  With w = weights
 * (NULL: all ones) and W = sum_i w_i:
 *   mean[e]       Euclidean entry: sum w x / W, evaluated as x_0 + sum w (x - x_0) / W (a constant column gives x_0 exactly);
 *                 circular entry (circular[e] != 0): atan2(S, C), C = sum w cos x / W, S = sum w sin x / W, reported in
 *                 [-pi, pi) (pi becomes -pi): scipy's circmean(high = pi, low = -pi).  Evaluated about the first point as
 *                 x_0 + atan2(S', C') with the sums of sin / cos (x - x_0): the same direction and length, and x_0 exactly
 *                 for a constant column;
 *   resultant[e]  hypot(C', S') = hypot(C, S), the mean resultant length in [0, 1], for a circular entry; NaN for a Euclidean one;
 *   cov           block b's d x d matrix at cov[cov_off]: sum w r_e r_f / W -- the POPULATION form (divided by W, not W - 1)
 *                 -- with r = x - mean for a Euclidean entry and r = wrap_pi(x - mean) in [-pi, pi) for a circular one.
 *                 For a circular entry this is the mean squared WRAPPED deviation about the circular mean (and the mean product
 *                 of wrapped deviations off the diagonal), not a variance about an arithmetic mean: the wrapped residuals need
 *                 not average to zero.  Two passes: the residuals are taken about the float64 mean, never sum x^2 - (sum x)^2.
 *   Xt[x_rows][n]: float32, device;  blocks[n_blocks]: HOST copy of the table (validated here), blocks_dev: DEVICE copy (what
 *   the kernel reads);  cols [n_entries] int32, circular [n_entries] uint8 (nullable), weights [n] float64 (nullable,
 *   non-negative, not all zero: W = 0 gives NaN), mean, resultant [n_entries], cov [cov_count]: DEVICE arrays.
 * Two launches: a 256-thread group per entry (thread t adds points t, t + 256, ...; a fixed shuffle tree; the four waves in
 * order), then a group per block (wave w owns every fourth product of the upper triangle; lane l adds points l, l + 64, ...;
 * the same tree).  The sum of a product depends on n, its two rows and their flags alone: the diagonal blocks of a pair's
 * matrix are the bits of its variables' own matrices.
 * NFISAM_ERR_ARG: a NULL pointer (circular and weights excepted), n, x_rows, n_entries, n_blocks or cov_count < 1, more than
 * 65535 blocks, a block with d outside 1 .. 16 or a matrix outside [0, cov_count).  The device arrays are not read on the host:
 * an entry whose row is outside [0, x_rows) has NaN mean and resultant, and a block that holds such an entry or whose entries
 * leave [0, n_entries) has an all-NaN matrix (nothing is read out of bounds, every other entry and block is untouched); the
 * Python binding refuses such tables before upload.  (Additive: ABI 1600.) */
int nfisam_sample_moments(const float* Xt, int x_rows, int n, const nfisam_moment_block* blocks, const nfisam_moment_block* blocks_dev,
                          int n_blocks, const int32_t* cols, int n_entries, const uint8_t* circular, const double* weights,
                          double* mean, double* resultant, double* cov, long long cov_count, nfisam_stream_t stream);

/* out[e][q] (double[n_entries][n_probs]) = the quantile at probs[q] of the n float64 keys of entry e: x for a Euclidean
 * entry, wrap_pi(x - center[e]) for a circular one (the caller passes the means of nfisam_sample_moments; NULL: 0).  numpy's
 * default "linear" rule on the sorted keys s: h = p (n - 1), s[floor h] + (h - floor h) (s[ceil h] - s[floor h]); where h is
 * an integer the key itself, bit for bit.  A circular entry reports center + quantile UNWRAPPED, so the ends of an interval
 * stay ordered and may lie outside [-pi, pi): the caller wraps for display.  No weights.  (What the reference's mean and
 * ellipse plots, built on Statistics.py:151-171, cannot show of a non-Gaussian posterior.)
 *   probs[n_probs]: HOST copy (validated here), probs_dev: DEVICE copy (what the kernel reads);  cols, circular (nullable),
 *   center (nullable) [n_entries], out: DEVICE arrays.
 * One launch: a 256-thread group per entry sorts the keys in dynamic LDS (bitonic, padded with +inf to the next power of two:
 * 8 bytes per padded point, so small draws keep several groups per CU).
 * NFISAM_ERR_ARG, before any launch: a NULL pointer (circular and center excepted), n, x_rows, n_entries or n_probs < 1,
 * n > NFISAM_QUANTILE_MAX_N, a probability outside [0, 1] (or NaN).  An entry whose row is outside [0, x_rows), or a device
 * probability outside [0, 1], yields NaN (nothing is read out of bounds).  (Additive: ABI 1600.) */
int nfisam_sample_quantiles(const float* Xt, int x_rows, int n, const int32_t* cols, int n_entries, const uint8_t* circular,
                            const double* center, const double* probs, const double* probs_dev, int n_probs, double* out,
                            nfisam_stream_t stream);

/* ---- posterior modes: mean-shift over every block's samples, then a merge (sample_modes.hip) -------------------------------
 * One mean and one covariance per variable put a bimodal posterior's estimate between its hypotheses (a landmark seen by
 * range only, a pose under ambiguous data association).  Here every point of the COLUMN-major float32 device matrix
 * Xt[x_rows][n] climbs the Gaussian kernel density estimate of its block, and the converged points are merged into modes.
 * The block table is that of nfisam_sample_mmd (entry e names the row cols[e] of Xt; block b is the run of entries
 * col_off .. col_off + d with its own bandwidth), with 1 <= d <= NFISAM_MODES_MAX_D.  For block b, with w = weights (NULL: all
 * ones):
 *     u_e(a, y) = scale_e * wrap_e(a_e - y_e)     (scale NULL: 1; wrap_e brings the difference into [-pi, pi) where wrap[e] is
 *                                                  set -- the sign convention of theta_to_pipi -- and is the identity otherwise)
 *     k_j(y)    = w_j * exp(-inv_two_sigma2 * sum_e u_e(x_j, y)^2)
 * ASCENT, one from every point i, y = x_i:  delta_e = sum_j k_j(y) wrap_e(x_je - y_e) / sum_j k_j(y);  y_e += delta_e, a
 * wrapped entry brought back into [-pi, pi): one iteration.  It stops when 2 inv_two_sigma2 sum_e (scale_e delta_e)^2 <= tol^2
 * (a shift of at most `tol` sigmas) or after max_iters iterations.  Where the denominator is 0 (a zero-weight start out of
 * reach of every weighted point) the start stays where it is, with density 0 and 0 iterations.  The shift form -- not a
 * weighted mean of coordinates -- is right across the +-pi seam, and a constant column stays exactly where it is (all its
 * differences are 0).  A column with scale 0 does not enter the distances; it is carried along by the others' weights.
 * MERGE, deterministic: among the unlabelled starts the one of largest final density (lowest index on ties) founds mode m at
 * its converged point; every unlabelled start whose converged point is within `merge` sigmas of it
 * (2 inv_two_sigma2 sum_e u_e^2 <= merge^2) takes label m; until no start is unlabelled or max_modes modes exist.  Starts left
 * over (and starts of NaN density) keep label -1.  How small `merge` may be is set by the ascent, not by rounding: an ascent
 * that contracts by a factor r per iteration and stops at a shift of `tol` sigmas is still up to tol * r / (1 - r) sigmas short
 * of its limit, so members of one mode can end that far apart (1e-5 sigma for tol = 1e-7 and r = 0.99, seen on a uniform
 * square); a radius below that splits modes.  The default 1e-2 leaves three orders of magnitude.
 * Outputs (DEVICE arrays):
 *   pos [n_entries][n]                 converged points, by ENTRY: blocks that share entries share these rows -- give every block
 *                                      its own entries (rows of Xt may repeat freely)
 *   dens [n_blocks][n]                 sum_j k_j(y_final) / sum_j w_j
 *   iters [n_blocks][n] int32          shifts applied; negated when the ascent stopped on max_iters without meeting tol
 *   labels [n_blocks][n] int32, n_modes [n_blocks] int32, unlabelled [n_blocks] int32
 *   mode_pos [n_blocks][max_modes][16], mode_dens, mode_mass [n_blocks][max_modes]   (slots >= n_modes: NaN);
 *                                      mode_mass = sum of w over the members / sum of w over all starts
 *   blocks[n_blocks]: HOST copy of the table (validated here), blocks_dev: DEVICE copy (what the kernels read); cols [n_entries]
 *   int32, scale [n_entries] double >= 0 (nullable), wrap [n_entries] uint8 (nullable), weights [n] double >= 0, not all zero
 *   (nullable): DEVICE arrays.
 * Float32 points in; every difference, exponent, sum and division is float64, by direct differences.  Two launches, no float
 * atomics: (1) a 256-thread group per (64 starts, block) runs ALL iterations of its starts -- one start per lane, the four
 * waves each taking a quarter of every 128-point chunk staged in LDS, the partial sums added in wave order; (2) a group per
 * block merges.  A start's sums depend on n, its block's rows and flags alone: two calls give the same bits, and a block's
 * results are the same bits alone, repeated, or anywhere in a table.
 * NFISAM_ERR_ARG, before any launch: a NULL pointer (scale, wrap and weights excepted), x_rows, n_entries or n_blocks < 1,
 * n < 0, more than 65535 blocks, a block of the host copy with d outside 1 .. 16 or inv_two_sigma2 not positive and finite,
 * max_iters < 1, tol < 0, merge <= 0 (or either not finite), max_modes outside 1 .. NFISAM_MODES_MAX_MODES.  n == 0 returns
 * NFISAM_OK and touches nothing.  The device arrays are not read on the host: a block of the device copy whose entries leave
 * [0, n_entries), that names a row outside [0, x_rows) or whose d is outside 1 .. 16 gets NaN pos (its entries inside the
 * table), dens and mode_*, labels -1, iters 0, n_modes 0 and unlabelled n; nothing is read out of bounds and every other
 * block is untouched -- as long as blocks own their entries: `pos` is stored by entry, so a bad block that shares entries
 * with a good one (the C entry permits it, the binding does not) overwrites those rows of the good block with NaN, in a race; the Python binding refuses such tables before upload.  (Additive: ABI 1600.) */
#define NFISAM_MODES_MAX_D      16   /* widest block (the mode table's row length) */
#define NFISAM_MODES_MAX_MODES  32   /* most modes per block */
int nfisam_sample_modes(const float* Xt, int x_rows, int n, const nfisam_mmd_block* blocks, const nfisam_mmd_block* blocks_dev,
                        int n_blocks, const int32_t* cols, int n_entries, const double* scale, const uint8_t* wrap,
                        const double* weights, int max_iters, double tol, double merge, int max_modes, double* pos, double* dens,
                        int32_t* iters, int32_t* labels, int32_t* n_modes, double* mode_pos, double* mode_dens, double* mode_mass,
                        int32_t* unlabelled, nfisam_stream_t stream);

/* The second launch of nfisam_sample_modes alone: `pos` and `dens` of an earlier call (same table, cols, scale, wrap, weights
 * and n) are merged again -- another radius, another max_modes -- without climbing again; labels, n_modes, mode_* and
 * unlabelled are rewritten (mode_* sized for THIS max_modes), pos and dens are only read.  The same bits as a full call with
 * these arguments.  x_rows only serves the row check that marks a bad block.  NFISAM_ERR_ARG as above for the arguments it
 * shares; n == 0 returns NFISAM_OK and touches nothing.  (Additive: ABI 1600.) */
int nfisam_sample_modes_merge(int x_rows, int n, const nfisam_mmd_block* blocks, const nfisam_mmd_block* blocks_dev, int n_blocks,
                              const int32_t* cols, int n_entries, const double* scale, const uint8_t* wrap, const double* weights,
                              double merge, int max_modes, const double* pos, const double* dens, int32_t* labels,
                              int32_t* n_modes, double* mode_pos, double* mode_dens, double* mode_mass, int32_t* unlabelled,
                              nfisam_stream_t stream);

/* ---- k nearest neighbours and ball counts: a selection over pairs of points (sample_knn.hip) -------------------------------
 * What differential entropy (Kozachenko-Leonenko), mutual information (Kraskov-Stoegbauer-Grassberger) and a two-sample KL
 * divergence (Wang-Kulkarni-Verdu) of a sample set are estimated from, for posteriors whose marginals are rings or have two
 * modes, where 1/2 log det(2 pi e Sigma) is wrong by nats.  They stand in for nothing of the reference: it has no entropy or
 * information measure (its src/utils/Statistics.py stops at MMD, RMSE and KSD).  The estimators are formed on the host
 * (utils/Statistics.py: knn_entropy, knn_mutual_information, knn_divergence) from what these two entries return.
 * Xt[x_rows][m] holds the QUERIES and Yt[y_rows][n] the POINTS (COLUMN-major float32 device matrices, the layout of the tree
 * walk's St; they may be the same matrix).  Entry e names row xcols[e] of Xt and row ycols[e] of Yt, as in nfisam_sample_mmd;
 * block b is the run of entries col_off .. col_off + d, 1 <= d <= NFISAM_KNN_MAX_D.  Blocks may overlap and repeat entries.
 * For query i and point j of block b
 *     u_e  = scale_e * wrap_e((double)x_ie - (double)y_je)    (scale NULL: 1; wrap_e brings the difference into [-pi, pi) where
 *                                                              wrap[e] is set -- wrap_pi, the sign convention of theta_to_pipi)
 *     dist = max_e |u_e|  (NFISAM_KNN_NORM_MAX)   or   sqrt(sum_e u_e^2), the sum in ascending e  (NFISAM_KNN_NORM_L2).
 * A NaN u_e makes the distance NaN under either norm.
 *
 * nfisam_sample_knn: for every query and block the k smallest distances to the n points, candidates ordered by (distance, j):
 * on equal distances the lower j comes first.
 *   dist [n_blocks][k][m] double, ascending in k;  idx [n_blocks][k][m] int32 (nullable): the j of each.
 *   Slots with no candidate hold +inf and index -1.  exclude_self != 0 skips the pair j == i (it requires m == n).  A NaN
 *   distance never enters a list -- a query with a NaN coordinate gets +inf / -1 throughout -- and neither does an infinite
 *   one, which could not be told from an empty slot.
 *   log_sum [n_blocks] double (nullable) = sum_i log(dist[b][k-1][i]) over the queries whose k-th distance is positive and
 *   finite, n_used [n_blocks] int32 (nullable) = how many queries that was; by a second small launch in the family's fixed
 *   order (thread t adds queries t, t + 256, ... ascending, wave_sum, waves_in_order; sample_common.h), no float atomics.
 * nfisam_sample_ball_count: count [n_blocks][m] int32, count[b][i] = #{ j : dist_b(x_i, y_j) < radius[blocks[b].radius_row][i] },
 *   radius [n_radius][m] double on the device.  The comparison is strict; a NaN or negative radius gives 0; exclude_self as
 *   above.  (The marginal counts of KSG-1 inside the joint block's k-th distance.)
 *   blocks[n_blocks]: HOST copy of the table (validated here), blocks_dev: DEVICE copy (what the kernels read); xcols, ycols
 *   [n_entries] int32, scale [n_entries] double (nullable), wrap [n_entries] uint8 (nullable): DEVICE arrays.
 * Float32 points in; the float64 difference of two float32 values is exact, so the max norm carries ONE rounding (by scale) and
 * no sum; L2 adds d products and a square root.  A 256-thread group per (64 queries, block), one query per lane; the four
 * waves each take 16 of every 64 points staged in LDS, a thread keeps its best k (distance, j) in registers, and the four
 * lists of a query are merged through LDS by (distance, j).  Two calls give the same bits; a block's results do not depend on
 * its place in the table, on other blocks or on repeated entries; a query's results do not depend on m.
 * NFISAM_ERR_ARG, before any launch: a NULL pointer (scale, wrap, idx, log_sum and n_used excepted); m, n, x_rows, y_rows,
 * n_entries or n_blocks < 1; more than 65535 blocks, or more than 65535 64-wide tiles of queries or of points; k outside
 * 1 .. NFISAM_KNN_MAX_K; an unknown norm; a block of the host copy with d outside 1 .. 16; exclude_self with m != n; n_radius
 * < 1 or a radius_row of the host copy outside [0, n_radius).  The device copy of the table is not trusted: a block whose
 * entries leave [0, n_entries), that names a row outside its matrix or whose d is outside 1 .. 16 (for the count: or whose
 * radius_row is outside [0, n_radius)) yields NaN dist, -1 idx, NaN log_sum, 0 n_used and -1 count; nothing is read out of
 * bounds and every other block is untouched.  The Python binding refuses such tables before upload.  (Additive: ABI 1600.) */
#define NFISAM_KNN_MAX_D     16   /* widest block */
#define NFISAM_KNN_MAX_K     16   /* most neighbours per query */
#define NFISAM_KNN_NORM_MAX  0    /* max_e |u_e| */
#define NFISAM_KNN_NORM_L2   1    /* sqrt(sum_e u_e^2) */
typedef struct nfisam_knn_block {
    int32_t col_off;           /* first entry of the block in xcols / ycols / scale / wrap */
    int32_t d;                 /* number of entries, 1 .. NFISAM_KNN_MAX_D */
    int32_t radius_row;        /* row of `radius` the block's queries take (read by nfisam_sample_ball_count alone) */
    int32_t reserved;
} nfisam_knn_block;
int nfisam_sample_knn(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n, int exclude_self,
                      const nfisam_knn_block* blocks, const nfisam_knn_block* blocks_dev, int n_blocks, const int32_t* xcols,
                      const int32_t* ycols, int n_entries, const double* scale, const uint8_t* wrap, int k, int norm, double* dist,
                      int32_t* idx, double* log_sum, int32_t* n_used, nfisam_stream_t stream);
int nfisam_sample_ball_count(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n, int exclude_self,
                             const nfisam_knn_block* blocks, const nfisam_knn_block* blocks_dev, int n_blocks, const int32_t* xcols,
                             const int32_t* ycols, int n_entries, const double* scale, const uint8_t* wrap, int norm,
                             const double* radius, int n_radius, int32_t* count, nfisam_stream_t stream);

/* ---- marginal densities at query points: a Gaussian kernel density estimate in logs (sample_density.hip) -------------------
 * The marginal posterior density itself, at points the caller chooses: what a marginal's curve on a grid, a map over the
 * plane, the negative log predictive density at the ground truth (NLPD) and the level of the smallest highest-density
 * region that holds it are formed from (utils/Statistics.py: density_bandwidth, sample_density_t, hpd_level).  The
 * reference's figures copy the sample matrix to the host and run scipy.stats.gaussian_kde per coordinate on a 500-point
 * grid (example/slam/ * /kde_plot_grid.py, traj_plot.py); nfisam_sample_modes evaluates such an estimate at its own converged
 * starts only.  Qt[q_rows][m] holds the QUERIES and Xt[x_rows][n] the SAMPLES (COLUMN-major float32 device matrices, the
 * layout of the tree walk's St; they may be the same matrix).  Entry e pairs row qcols[e] of Qt with row xcols[e] of Xt, as
 * in nfisam_sample_knn; block b is the run of entries col_off .. col_off + d, 1 <= d <= NFISAM_DENSITY_MAX_D, with its own
 * bandwidth matrix H given as the lower-triangular W with W H W' = I (W = inv(chol(H))).  Blocks may overlap and repeat
 * entries: that is how bandwidth candidates share one launch.  For block b, query i and sample j
 *     diff_c = (double)x_jc - (double)q_ic          (brought into [-pi, pi) by the wrap of sample_common.h where wrap[e] is set)
 *     u_r    = sum_{c <= r} W_rc diff_c             (c ascending, fma)
 *     e_ij   = -1/2 sum_r u_r^2 + log_w[j]          (log_w NULL: 0; a -inf entry -- a zero weight -- never contributes)
 *     log_dens[b][i] = ((log_norm + M_i) + log(sum_j exp(e_ij - M_i))) - log W_tot,        M_i = max_j e_ij,
 * W_tot = exp(log_w_sum) (n for NULL log_w), less w_i = exp(log_w[i]) under exclude_self; without exclude_self log W_tot is
 * log_w_sum itself.  exclude_self != 0 skips j == i (it requires m == n): the leave-one-out density.
 *   log_dens [n_blocks][m] double; dens [n_blocks][m] double (nullable) = exp(log_dens).
 *   A query whose every e_ij is -inf (n = 1 under exclude_self; zero weights only) gets log_dens = -inf and dens = 0.  A query
 *   with a NaN coordinate in the block gets NaN: the max keeps a NaN.  A query 1e4 bandwidths from every sample gets a finite
 *   log_dens (about -5e7) and dens = 0: the shift by M_i is what makes the log usable in tails.
 *   On a circular entry the NEAREST IMAGE alone is summed: a kernel wider than pi / 3 (1 / W_rr) puts more than 0.27 % of its
 *   mass past the seam, and the Python binding refuses it.
 *   blocks[n_blocks]: HOST copy of the table (validated here), blocks_dev: DEVICE copy (what the kernel reads); qcols, xcols
 *   [n_entries] int32, wrap [n_entries] uint8 (nullable), log_w [n] double (nullable): DEVICE arrays.
 * Float32 points in, float64 everywhere else.  A 256-thread group per (64 queries, block), one query per lane; the samples
 * are walked twice in chunks of 128 staged in LDS, the four waves a quarter each: first the max, then the sum of exp(e - M)
 * -- a thread's j ascending, then the four waves in order (sample_common.h); one float64 exp per pair, no float atomics.
 * Two calls give the same bits; a block's rows are the same bits alone, repeated, or anywhere in a table; a query's result
 * does not depend on m.
 * NFISAM_ERR_ARG, before any launch: a NULL pointer (wrap, log_w and dens excepted); m, n, q_rows, x_rows, n_entries or
 * n_blocks < 1; more than 65535 blocks or 64-wide tiles of queries; exclude_self with m != n; log_w with a log_w_sum that is
 * not finite; a block of the host copy with d outside 1 .. 6, a log_norm or whiten entry that is not finite, or a diagonal
 * entry <= 0.  The device copy of the table is not trusted: a block whose entries leave [0, n_entries), that names a row
 * outside its matrix or whose d is outside 1 .. 6 yields NaN for its rows of log_dens and dens; nothing is read out of bounds
 * and every other block is untouched.  The Python binding refuses such tables before upload.  (Additive: ABI 1600.) */
#define NFISAM_DENSITY_MAX_D 6            /* a pair of SE(2) variables; a KDE means nothing wider at n ~ 2000 */
typedef struct nfisam_density_block {
    int32_t col_off;      /* first entry of the block in qcols / xcols / wrap */
    int32_t d;            /* 1 .. NFISAM_DENSITY_MAX_D */
    double  log_norm;     /* sum_r log W_rr - d/2 log(2 pi), supplied by the host */
    double  whiten[21];   /* W: lower triangle, row-major packed, d(d+1)/2 used; W H W' = I for bandwidth matrix H */
} nfisam_density_block;
int nfisam_sample_density(const float* Qt, int q_rows, int m, const float* Xt, int x_rows, int n, int exclude_self,
                          const nfisam_density_block* blocks, const nfisam_density_block* blocks_dev, int n_blocks,
                          const int32_t* qcols, const int32_t* xcols, int n_entries, const uint8_t* wrap,
                          const double* log_w, double log_w_sum, double* log_dens, double* dens, nfisam_stream_t stream);

/* ---- trajectory error of every sample against ground truth: aligned ATE and RPE (sample_trajectory.hip) -------------------
 * The figure SLAM work is judged by, for every row of the sample matrix instead of for the posterior mean alone.  The
 * reference grades one trajectory on the host: its Plaza scripts copy the samples out, take the mean, align it to the truth
 * with `kabsch_umeyama` (src/utils/Functions.py:53-71, an SVD) and report the RMSE that is left
 * (example/slam/plaza_dataset/plaza_traj_performance_plot.py:112-114,196-198,282-293).  Xt[x_rows][n] is the COLUMN-major
 * float32 device matrix of the tree walk (the layout of nfisam_sample_moments); a lane carries one sample.
 * The table: P entries, one per pose or landmark.  Entry e names the rows col_x, col_y, col_th of Xt (col_th = -1: no
 * heading) and holds the float64 truth ax, ay, ath; flags bit 0 (NFISAM_TRAJ_ALIGNED): the entry takes part in the
 * alignment; bit 1 (NFISAM_TRAJ_LANDMARK): its squared residual goes to the landmark sum, not to the trajectory's. */
#define NFISAM_TRAJ_ALIGNED  1
#define NFISAM_TRAJ_LANDMARK 2
#define NFISAM_TRAJ_ALIGN_NONE       0
#define NFISAM_TRAJ_ALIGN_RIGID      1
#define NFISAM_TRAJ_ALIGN_SIMILARITY 2
#define NFISAM_TRAJ_OUT_ROWS 8
typedef struct nfisam_traj_entry {
    int32_t col_x, col_y;      /* rows of Xt */
    int32_t col_th;            /* row of the heading, or -1 */
    int32_t flags;             /* NFISAM_TRAJ_ALIGNED | NFISAM_TRAJ_LANDMARK */
    double  ax, ay, ath;       /* ground truth (ath is not read where col_th = -1) */
} nfisam_traj_entry;
typedef struct nfisam_traj_pair {
    int32_t i, j;              /* two entries that have headings: the pose j is seen from the pose i */
    int32_t slot;              /* which sum the pair goes to, 0 .. n_slots - 1 (one slot per stride) */
    int32_t reserved;
} nfisam_traj_pair;

/* nfisam_sample_trajectory_error replaces Functions.py:53-71 and plaza_traj_performance_plot.py:112-114,196-198,282-293, per
 * sample.  Over the aligned entries, with a', b' the truth and the sample about their centroids a_bar, b_bar:
 *     dot = sum a'.b',  cross = sum (a'_y b'_x - a'_x b'_y),  g = hypot(dot, cross),  theta = atan2(cross, dot)
 *     mode NONE: theta = 0, c = 1, t = 0;  RIGID: c = 1;  SIMILARITY: c = g / sum |b'|^2 (the least-squares scale);
 *     t = a_bar - c R(theta) b_bar in both aligned modes.
 *   reflect != 0: the improper fit R(phi) diag(1, -1), phi = atan2(cross-, dot-), dot- = sum (a'_x b'_x - a'_y b'_y),
 *   cross- = sum (a'_x b'_y + a'_y b'_x), is taken when hypot(dot-, cross-) > g; a heading h then maps to phi - h and theta
 *   reports phi.  g == 0 (one aligned entry, coincident points) gives theta = 0; sum |b'|^2 == 0 gives c = 1.  This is the
 *   SVD route's result with S = diag(1, d).  Two passes throughout: never sum x^2 - (sum x)^2 on raw coordinates.
 *   A second sweep forms the residuals r_e = a_e - (c R b_e + t).
 *   out  [NFISAM_TRAJ_OUT_ROWS][n] double: theta, c, t_x, t_y, sum |r|^2 over the entries without NFISAM_TRAJ_LANDMARK, the
 *        same over those with it, sum wrap_pi(b_th + theta - a_th)^2 over the entries with a heading, the largest |r_e| over
 *        the trajectory entries (NaN if there is none).  (The entry counts are the table's.)
 *   iout [2][n] int32: 1 where the improper fit was taken; the entry of that largest residual (the first of equal ones; -1).
 *   entry_sums [P + 1] double: sum_i w_i |r_e,i|^2 for every entry, then sum_i w_i (weights [n] double, NULL: all ones).
 *   scratch: nfisam_sample_trajectory_scratch_count(n, P) doubles.
 *   entries: HOST copy of the table (validated here); entries_dev: DEVICE copy (what the kernels read).
 * Float32 points in, float64 everywhere else; no float atomics.  A 256-thread group per 64 samples: a sample per lane, wave w
 * takes the entries w, w + 4, ..., the four waves' sums meet in wave order; the per-entry sums take a wave_sum per tile and a
 * second launch that adds the tiles in ascending order.  Two calls give the same bits; a sample's row of out / iout depends on
 * its own column and the table alone, not on n or the other samples.  A NaN or infinite coordinate of a sample makes every
 * output of that sample NaN (iout: 0, -1) and the entry sums, which add over samples; no other sample changes.
 * NFISAM_ERR_ARG, before any launch: a NULL pointer (weights excepted); x_rows, n or P < 1; an unknown mode; an entry of the
 * host copy with a row outside [0, x_rows) (col_th: [-1, x_rows)), an unknown flag or a truth that is not finite; an aligned
 * mode without an aligned entry.  A row of the DEVICE copy outside the matrix is never read and yields NaN.
 * (Additive: ABI 1600.) */
size_t nfisam_sample_trajectory_scratch_count(int n, int P);
int nfisam_sample_trajectory_error(const float* Xt, int x_rows, int n, const nfisam_traj_entry* entries,
                                   const nfisam_traj_entry* entries_dev, int P, int mode, int reflect, const double* weights,
                                   double* out, int32_t* iout, double* entry_sums, double* scratch, nfisam_stream_t stream);

/* Relative pose error, the gauge-free companion (no alignment; in the reference nowhere: its scripts stop at
 * plaza_traj_performance_plot.py:282-293).  For a pair (i, j) of entries with headings, from the sample and from the truth
 * alike:  d = R(-th_i) (p_j - p_i),  dth = wrap_pi(th_j - th_i).
 *   out [n_slots][2][n] double: per slot and sample, sum |d_est - d_true|^2 and sum wrap_pi(dth_est - dth_true)^2 over the
 *   slot's pairs (their count is the table's).  One launch serves every slot: a group per (64 samples, slot), wave w takes the
 *   pairs w, w + 4, ... of the table and skips other slots'.  The same promises as above.
 * NFISAM_ERR_ARG, before any launch: a NULL pointer; x_rows, n, P, n_pairs or n_slots < 1; more than 65535 slots; a bad entry
 * (as above); a pair of the host copy that names an entry outside [0, P), an entry without a heading or a slot outside
 * [0, n_slots).  (Additive: ABI 1600.) */
int nfisam_sample_trajectory_rpe(const float* Xt, int x_rows, int n, const nfisam_traj_entry* entries,
                                 const nfisam_traj_entry* entries_dev, int P, const nfisam_traj_pair* pairs,
                                 const nfisam_traj_pair* pairs_dev, int n_pairs, int n_slots, double* out, nfisam_stream_t stream);

/* ---- training -------------------------------------------------------------------------- */
/* Vector-Jacobian product of the L-layer flow (what torch autograd computes for
 * `loss.backward()` in slam/NFiSAM.py:474): kgrad[L*kparam_count] += d<gz,z>/dtheta + d<gl,logdet>/dtheta,
 * gx[n,D] (nullable) = the same w.r.t. x.  nll_mode=1 ignores gz/gl and uses
 * sum_p(0.5|z_p|^2 - logdet_p) (the un-normalised NLL of NFiSAM.py:470-472; divide by n and add
 * D/2 log 2pi for the reference's loss); loss_sum[1] += that sum (nullable).
 * kgrad / loss_sum are ACCUMULATED into (caller zeroes them).                               */
int nfisam_nsf_backward(const float* x, const float* kparams, int n, int D, int K, int H, float B, int L,
                        size_t layer_stride, const float* gz, const float* gl, int nll_mode, float* kgrad,
                        float* gx, float* loss_sum, nfisam_stream_t stream);

/* Device-resident control block of one clique's training run. */
typedef struct nfisam_train_state {      /* 32 bytes since ABI 1200 (the unused loss_acc / loss_slots[64] of ABI 1100 are gone);
                                          * ABI 1300: reserved[0] of a plan's host mirror counts the chunks closed in the current run */
    int32_t step;        /* iterations completed and recorded so far (advances when a chunk is closed) */
    int32_t stop;        /* set by the device when the early-stop rule fired                 */
    int32_t have_avg;    /* a previous window mean exists                                    */
    float   loss_avg;    /* previous window mean (NFiSAM.py:481-491)                         */
    int32_t domain_err;  /* bit 0: a kernel saw a non-finite loss; bit 1 (NFISAM_STATE_STALLED, ABI 1400): a group
                          * barrier of a chunk-persistent launch timed out (-> NFISAM_ERR_STALL)            */
    int32_t reserved[3]; /* [0]: a plan's host mirror counts the chunks closed in the current run; [1] (ABI 1400): the
                          * most XCDs one (clique, dim) group of a chunk-persistent launch ran on (1 = the placement the
                          * grid asks for; diagnostic, correctness does not depend on it)                   */
} nfisam_train_state;

#define NFISAM_STATE_STALLED 2

typedef struct nfisam_adam_cfg {
    float lr, beta1, beta2, eps;      /* torch.optim.Adam defaults: betas .9/.999, eps 1e-8 (NFiSAM.py:425) */
    int32_t max_iters;                /* flow_iterations                                      */
    int32_t average_window;           /* <=0 disables early stopping                          */
    float loss_delta_tol;
    int32_t reserved;
} nfisam_adam_cfg;

/* One clique of a training batch: everything device-resident. */
typedef struct nfisam_clique {
    const float* x;              /* [n,D] normalised training batch (NFiSAM.py:379)           */
    float* kparams;              /* [L*kparam_count]                                          */
    float* adam_m;               /* [L*kparam_count] zero-initialised                         */
    float* adam_v;               /* [L*kparam_count] zero-initialised                         */
    float* kgrad;                /* [nfisam_nsf_grad_workspace_count(max n of the batch, D,..)] workspace, zero-initialised --
                                  * and ZEROED AGAIN by the caller whenever it resets `state` (step = 0) to re-run a plan: the
                                  * chunk-persistent kernel's blocks exchange gradient words as (value, tag) pairs whose tag is
                                  * the iteration's number in the run (state->step + i + 1), so a workspace that still holds the
                                  * pairs of an earlier run with the same numbering would be read as this run's (ABI 1400)     */
    float* iter_loss;            /* [max_iters] zero-initialised; per-iteration loss (NFiSAM.py:473) */
    nfisam_train_state* state;   /* zero-initialised                                          */
    int32_t n, D;
} nfisam_clique;

/* Floats the `kgrad` workspace of a clique must hold (gradient copies + a ring of 128 x 128 per-iteration
 * loss words behind them -- ABI 1600; 128 x 64 before: a lone clique of up to 256 blocks keeps two blocks per word, an
 * order-free sum -- + 64 counter words: the per-dim group barriers of the chunk-persistent training
 * kernel, which the library keeps zero between chunks -- the caller provides the workspace ZEROED) when the largest clique of its batch has n
 * particles: launches of <= 128 particle tiles write per-tile partial gradients with plain stores and
 * the Adam kernel sums them in tile order (no atomics); larger ones accumulate with float atomics
 * into a single copy.  A tile is 32 particles (two-lanes-per-particle kernel) or 64 (one lane per
 * particle; the dim-major kernel of one-layer flows writes one copy per block of 4 waves); the count is
 * the upper bound of all, plus -- for one-layer flows of <= 32 tiles of 64 -- the second set of copies
 * and the second (theta | m | v) buffer of the launches that apply the previous iteration's Adam update
 * themselves (nfisam_nsf_train_plan_run; no separate Adam launch per iteration); for multi-layer flows
 * of hidden width 8 and D <= 16 (ABI 1310) the clique's PANEL IMAGE (the parameters in the order the
 * multi-layer training kernel reads them from LDS, L x D panels; the Adam kernel keeps it current)
 * and, for latency-bound sizes, the forward state that kernel parks between its two passes.
 * Always allocate what this function returns -- the layout behind the gradient copies is the library's. */
size_t nfisam_nsf_grad_workspace_count(int n, int D, int K, int H, int L);

/* The gradient half of a training iteration on its own (forward + analytic backward + reduction into
 * each clique's `kgrad` workspace and loss slots, exactly the kernel `nfisam_nsf_train_step` launches
 * first; no Adam update, no bookkeeping, state->stop / step are still honoured).  With <= 128 tiles the
 * workspace is overwritten (per-tile slabs), so repeated calls are idempotent: bench.py times this
 * entry to price the dominant kernel; callers with their own optimiser use it as the gradient oracle. */
int nfisam_nsf_train_gradient(const nfisam_clique* cliques, int n_cliques, int cliques_on_host, int max_n,
                              int max_D, int K, int H, float B, int L, nfisam_stream_t stream);

/* Training plans split an iteration of a one-layer batch into `nfisam_nsf_train_chains(...)` launches that run as
 * parallel branches of the chunk's hipGraph (the (clique, dim) groups of a one-layer flow are independent optimisation
 * problems, reference loop src/slam/NFiSAM.py:451-494; a branch's kernel prologue and tail then run under another
 * branch's arithmetic).  `nfisam_nsf_train_gradient_part` is launch `chain` of `n_chains` of the gradient half, for
 * callers that want to time or drive the launches exactly as a plan issues them (bench.py: one stream per chain).
 * n_chains = 1 is nfisam_nsf_train_gradient.  Launch shapes that are not split return 1 from nfisam_nsf_train_chains
 * and NFISAM_ERR_ARG for n_chains > 1. */
int nfisam_nsf_train_chains(int n_cliques, int max_n, int max_D, int K, int H, int L);
int nfisam_nsf_train_gradient_part(const nfisam_clique* cliques, int n_cliques, int cliques_on_host, int max_n,
                                   int max_D, int K, int H, float B, int L, int chain, int n_chains,
                                   nfisam_stream_t stream);

/* One full-batch training iteration of `n_cliques` independent cliques (grid.y = clique):
 * forward + analytic backward + gradient reduction, the Adam update, and a one-wave bookkeeping kernel
 * that records iter_loss[step], evaluates the reference's window early-stop rule on the device and
 * advances state->step.  Cliques whose state->stop is set or whose step reached max_iters are skipped,
 * so the call can be replayed without host intervention.
 * `cliques` is a DEVICE array unless n_cliques==1 and `cliques_on_host` is non-zero.
 * All cliques share K, H, B, L and the Adam configuration; n and D may differ.             */
int nfisam_nsf_train_step(const nfisam_clique* cliques, int n_cliques, int cliques_on_host, int max_n,
                          int max_D, int K, int H, float B, int L, const nfisam_adam_cfg* cfg,
                          nfisam_stream_t stream);

/* Convenience loop == the `for i in range(flow_iterations)` loop of NFiSAM.fit_clique_density_model
 * (slam/NFiSAM.py:451-491) for a batch of independent cliques.  Enqueues iterations in chunks (the
 * largest divisor of `average_window` that is <= 128; 50 without early stopping): 2 kernels per iteration
 * plus one bookkeeping kernel per chunk -- the only writer of state->step / stop -- captured once as a
 * hipGraph and replayed, and SYNCHRONISES WITH THE HOST after each chunk to read the stop flags.  host_cliques: HOST array of descriptors (device pointers
 * inside); dev_cliques: the same array in device memory.  iters_run[n_cliques] (host) receives the
 * iterations each clique ran.                                                                */
int nfisam_nsf_train_loop(const nfisam_clique* host_cliques, const nfisam_clique* dev_cliques, int n_cliques,
                          int K, int H, float B, int L, const nfisam_adam_cfg* cfg, int use_graph,
                          int32_t* iters_run, nfisam_stream_t stream);

/* The same loop with the set-up split off, so that descriptor validation and hipGraph capture /
 * instantiation happen once (outside any timed region) and the plan can be re-run, e.g. after the
 * caller re-initialised parameters / Adam moments / state in place.  `plan_run` synchronises with
 * the host after every chunk of `average_window` (50 if early stopping is off) iterations.
 * Re-running a plan from step 0: re-initialise parameters, moments, `iter_loss`, `state` AND the `kgrad` workspace (zero) --
 * see nfisam_clique.kgrad; continuing a run (state left as it is) needs nothing.                 */
typedef struct nfisam_train_plan nfisam_train_plan;
int nfisam_nsf_train_plan_create(const nfisam_clique* host_cliques, const nfisam_clique* dev_cliques, int n_cliques,
                                 int K, int H, float B, int L, const nfisam_adam_cfg* cfg, int use_graph,
                                 nfisam_train_plan** out);
int nfisam_nsf_train_plan_run(nfisam_train_plan* plan, int32_t* iters_run, nfisam_stream_t stream);
/* ABI 1400, measurement only.  A plan created with `use_graph = 3` (graph | timing) splits a chunk-persistent chunk into two
 * graphs -- the training launch(es), then the closing Adam update + bookkeeping -- and records two timing events on the
 * stream around the first: after a run and a synchronisation, `ms` = GPU time of the persistent launch(es) of the most
 * recent chunk (bench.py's `roofline.kernel_us`).  One more graph launch per chunk: not for production plans.
 * NFISAM_ERR_ARG for plans without the events, NFISAM_ERR_LAUNCH when no persistent chunk has run. */
int nfisam_nsf_train_plan_kernel_ms(const nfisam_train_plan* plan, float* ms);
int nfisam_nsf_train_plan_destroy(nfisam_train_plan* plan);

/* Stepping a graph plan by hand (ABI 1320; the slot scheduler of slam/ReplicaNFiSAM.py: independent runs whose cliques
 * enter and leave ONE batched launch sequence as they finish -- the reference trains the cliques of its eight dataset
 * variants one after the other, example/slam/plaza_dataset/run_nfisam.py:11-21):
 *   begin    orders the plan's stream behind `stream` and restarts the chunk count of the host mirror;
 *   enqueue  appends ONE chunk of `average_window` iterations (non-blocking: enqueue a few ahead);
 *   peek     copies the host mirror, out[n_cliques]: each clique's state as of the last chunk closed and, in
 *            reserved[0], the number of chunks closed since `begin` (-1: a chunk closed during the copy, look again);
 *   stream   the plan's stream: a clique that has stopped (or reached max_iters) is not written by any launch any more,
 *            so the caller may re-initialise its slot for a NEW problem of the same (n, D) -- batch, parameters, zeroed
 *            moments / workspace / loss record and, LAST, the zeroed state -- with copies enqueued on this stream, i.e.
 *            between two chunks;
 *   refill   does exactly that for slot `clique` from the caller's device buffers x [n,D] / kparams (ordered behind
 *            `stream`; they must stay alive until the copies have run);
 *   feed     a thread of the library keeps `depth` chunks enqueued ahead of the last one closed, so that the caller's
 *            thread never sits in the graph launch (~0.3 ms per chunk); depth 0 pauses it (returns once it is outside a
 *            launch); `enqueued` = chunks enqueued since `begin`: a slot refilled when this read E trains from chunk
 *            E + 1 on at the latest, i.e. its mirror entry is its own once more than E chunks have closed;
 *   end      pauses the feeder and orders `stream` behind everything enqueued on the plan.                */
int nfisam_nsf_train_plan_begin(nfisam_train_plan* plan, nfisam_stream_t stream);
int nfisam_nsf_train_plan_enqueue(nfisam_train_plan* plan);
/* ABI 1400.  A training plan with the reference's HOLD-OUT stop rule (src/slam/NFiSAM.py:452-468, `training_set_frac < 1`):
 * every `validation_interval` iterations -- in front of iteration i whenever (i + 1) % validation_interval == 0 -- the
 * negative mean log-density of the held-out batch under the current parameters is evaluated on the device; the first time
 * it exceeds the previous evaluation the run is scheduled to end at slower_stop_iter = int(slower_stop_rate * (i + 1))
 * (the loop breaks in front of the iteration with i + 1 >= slower_stop_iter) and evaluation ceases.  The window rule is
 * off in this mode (cfg->average_window is ignored), as in the reference (`if testing_data is None`, :481).
 * One graph replay = one validation period; whole-number slower_stop_rate >= 1 only (the reference's default 2.0: the
 * scheduled end then falls on a period boundary), 1 <= validation_interval <= 129; anything else: NFISAM_ERR_ARG (callers
 * step such fits themselves).  state->have_avg / loss_avg hold the last validation loss, state->reserved[2] the scheduled
 * end (0: none).  `val[c].logprob` is scratch of n_val floats; `val[c].val_loss` (nullable) receives evaluation number k
 * at index k (max_iters / validation_interval entries).  All device pointers; `val` itself is a host array. */
typedef struct nfisam_validation {
    const float* x_val;       /* [n_val, D] held-out batch, normalised as the reference does (its OWN statistics, NFiSAM.py:381) */
    float* logprob;           /* [n_val] scratch                                                              */
    float* val_loss;          /* [max_iters / validation_interval] or NULL                                    */
    int32_t n_val;
    int32_t reserved;
} nfisam_validation;
int nfisam_nsf_train_plan_create_validated(const nfisam_clique* host_cliques, const nfisam_clique* dev_cliques, int n_cliques,
                                           int K, int H, float B, int L, const nfisam_adam_cfg* cfg,
                                           const nfisam_validation* val, int validation_interval, float slower_stop_rate,
                                           int use_graph, nfisam_train_plan** out);

/* ABI 1400.  Most XCDs one (clique, dim) group of the plan's chunk-persistent launches ran on (0: none has run; 1: what
 * the grid asks for; > 1: slower, equally correct -- the group's exchange uses agent-scope write-through stores).  */
int nfisam_nsf_train_plan_xcd_span(const nfisam_train_plan* plan);

/* ABI 1600 (round 6), not in the reference: the whole run of a SINGLE-CLIQUE plan enqueued on `stream` as one window-spanning launch
 * that evaluates the reference's window rule (src/slam/NFiSAM.py:481-491) itself, without the host -- the call returns at once.  The
 * plan must have been created with bit 2 (value 4) of `use_graph` set.  Outcome, once the stream has drained: `state->step` =
 * iterations run, `state->stop`, `state->domain_err` (bit 0 non-finite loss, NFISAM_STATE_STALLED), `iter_loss`; parameters and moments
 * are the trained ones -- the same bits nfisam_nsf_train_plan_run leaves.  -> NFISAM_ERR_ARG: this plan / this moment does not allow
 * it (no such graph; hidden_dim or width without the two-wave build; another run holds the chunk-persistent form): use
 * nfisam_nsf_train_plan_run. */
int nfisam_nsf_train_plan_launch_async(nfisam_train_plan* plan, nfisam_stream_t stream);
int nfisam_nsf_train_plan_feed(nfisam_train_plan* plan, int depth);
long nfisam_nsf_train_plan_enqueued(const nfisam_train_plan* plan);
int nfisam_nsf_train_plan_peek(const nfisam_train_plan* plan, nfisam_train_state* out);
nfisam_stream_t nfisam_nsf_train_plan_stream(nfisam_train_plan* plan);
int nfisam_nsf_train_plan_refill(nfisam_train_plan* plan, int clique, const float* x, const float* kparams,
                                 nfisam_stream_t stream);
int nfisam_nsf_train_plan_end(nfisam_train_plan* plan, nfisam_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFISAM_HIP_H */
