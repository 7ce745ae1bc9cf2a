/*
 * irec.h -- C ABI of libirec_hip.so: the MI355X-native iREC beam-search coder.
 *
 * This is the drop-in boundary for the hot path of gergely-flamich/relative-entropy-coding:
 *   rec/coding/beam_search_coder.py  BeamSearchCoder.encode_block / decode_block
 *   rec/coding/coder.py              GaussianCoder.encode / decode, Coder.split / merge
 * Plain pointers and sizes only; no torch / HIP types in the signatures (a HIP stream is passed as void*).
 *
 * Conventions
 *   - "device pointer" arguments must point to memory of the HIP device the context was created on.
 *   - Device entry points are ASYNCHRONOUS on the given stream; they never allocate, free or synchronise.
 *   - The library keeps no hidden mutable state besides the read-only constant tables of a context
 *     (the reference mutates TF's process-global RNG on every call: beam_search_coder.py:38, coder.py:62,111).
 *   - Every function returns an irec_status (0 = ok, negative = error); irec_last_error() gives the text
 *     of the calling thread's last error.
 *
 * Blocks.  A "block" is one <= block_size slice of a shuffled latent tensor (coder.py:69-83).  For block k:
 *     element i (0 <= i < block_dim[k]) lives at flat index
 *         block_base[k] + ( perm ? perm[block_pos[k] + i] : block_pos[k] + i )
 *     of q_loc / q_scale / p_loc / p_scale / out_sample, where block_base[k] is the offset of the block's tensor
 *     inside the concatenated arrays, block_pos[k] the block's start inside the shuffled tensor and perm the
 *     tf.random.shuffle permutation of that tensor size (irec_tf_shuffle_perm), shared by all tensors of the call.
 *     Reading through perm IS Coder.split; writing out_sample through it IS Coder.merge.
 */
#ifndef IREC_H_
#define IREC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IREC_BIG_PRIME 10007     /* beam_search_coder.py:30 */
#define IREC_MAX_BEAMS 256       /* hard limit of this build (reference: any python int, beam_search_coder.py:28); B <= 60 takes the */
                                 /* register-resident encoders, anything above the generic kernel                                    */
#define IREC_MAX_PARTITIONS 65536 /* hard limit on K = ceil(KL / kl_per_partition) */
/* Seeds.  A CODING SEED is the `seed` of GaussianCoder.encode / decode: any int64 up to IREC_SEED_MAX = INT64_MAX -
 * (IREC_MAX_PARTITIONS + 2), so that no step seed the library forms from it -- seed + t of step t < IREC_MAX_PARTITIONS, seed + j + 1
 * and seed + j + 2 of the Gumbel draw of step j -- overflows int64.  Every entry point that takes a coding seed (irec_beam_encode[_ex],
 * irec_beam_decode[_ws | _tensors], irec_normal_table_build, irec_gumbel_table_build, irec_test_proposal_table) answers IREC_E_INVALID
 * above it, with the seed and the bound in irec_last_error(); nothing is launched and nothing is written.  The host sampler
 * (irec_importance_encode / _decode, irec_tf_stateless_gumbel) takes the seed of ONE step, which its caller forms from a coding seed,
 * and adds at most 2 to it: it answers IREC_E_INVALID above INT64_MAX - 2.  Negative seeds are valid.  The beam-search coders reduce seed + t modulo 2^31 - 1
 * (TensorFlow's truncation of both seeds, python/framework/random_seed.py; residue 0 becomes the pair (0, 2^31 - 1)), so seeds congruent
 * modulo 2^31 - 1 code identically -- as they do in the reference; the shuffle and the importance coder's normal stream take their op
 * seed from CPython's random.Random(seed), which sees every bit of the seed.  The stamps of IREC_FLAG_REUSE_TABLES hold all 64 bits: two
 * seeds share a table only if they are equal.
 * A HEADER SEED is the uint32 field of a .rec / .recs file (irec_rec_encode_file*): a file can only name a coding seed in [0, 2^32), and
 * decompress codes under the seed it reads, so a caller that writes files must code under a seed of that range (irec.io.header_seed
 * refuses any other before a byte is written). */
#define IREC_SEED_MAX (INT64_MAX - (IREC_MAX_PARTITIONS + 2))

typedef enum {
  IREC_OK = 0,
  IREC_E_INVALID = -1,     /* bad argument (null pointer, non-positive size, B > IREC_MAX_BEAMS ...)            */
  IREC_E_HIP = -2,         /* a HIP runtime call failed; text in irec_last_error()                             */
  IREC_E_NO_DEVICE = -3,   /* no usable gfx950 device: the library has NO CPU fallback                         */
  IREC_E_WORKSPACE = -4    /* workspace smaller than irec_encode_workspace_bytes()                             */
} irec_status;

/* Constructor arguments of BeamSearchCoder (beam_search_coder.py:15-30) after its own preprocessing. */
typedef struct {
  float kl_per_partition; /* Omega, stored as float32 by GaussianCoder.__init__ (coder.py:192)                 */
  int32_t n_samples;      /* S = int(exp(kl_per_partition * extra_samples)) (beam_search_coder.py:29)          */
  int32_t n_beams;        /* B (beam_search_coder.py:28)                                                       */
  int32_t flags;          /* IREC_FLAG_* below; 0 = defaults                                                   */
  int32_t table_dims[4];  /* optional hint: the distinct block_dim values of the call (0-terminated, <= 4).     */
                          /* With it the encoder evaluates the shared-seed Philox draw once per call into a     */
                          /* proposal table (same seed for every block, coder.py:444-449) instead of once per   */
                          /* block; a block whose dim is not listed gets out_K = -1.  All zero = no hint.       */
  int32_t table_steps;    /* partitions the proposal tables cover (0 = IREC_TABLE_STEPS_DEFAULT), clamped to    */
                          /* [1, min(max_K, IREC_TABLE_STEPS_MAX)] and to what IREC_TABLE_BYTES_MAX holds of the */
                          /* call's tables (2 * S * sum of the table dims bytes per step; at least               */
                          /* IREC_TABLE_STEPS_FLOOR steps within IREC_TABLE_BYTES_HARD).  Table scratch is       */
                          /* O(table_steps * S * D): a block with more partitions is coded by the fused-Philox   */
                          /* kernel in a second pass of the same call (blocks of more than 1024 dims: inside the */
                          /* chunked encoder, which draws the rows of those steps itself) -- same outputs.       */
} irec_params;

#define IREC_FLAG_FORCE_GENERIC 1 /* use the generic (any D, any B) kernel even where the fast kernels apply   */
#define IREC_FLAG_NO_SPLIT 16     /* no block is shared: neither the split encoder (several workgroups per block for calls of few     */
                                  /* blocks) nor shared rows between teams (calls of one to 1.5 blocks per CU, B > 10) nor gangs of   */
                                  /* teams (calls of at most 384 blocks of more than 1024 dims: several teams per block)              */
#define IREC_FLAG_TABLES_PRESENT 65536 /* stronger than REUSE_TABLES: the caller vouches that the PREVIOUS irec_beam_encode call on this  */
                                  /* workspace and stream was this call's twin (same seed, S, table_dims, table window, table kind --  */
                                  /* e.g. the next residual block of the same image) and that nothing has run on the workspace since:   */
                                  /* the table kernels are not even launched (two launches fewer per call of a latency-bound pass).     */
#define IREC_FLAG_REUSE_TABLES 64 /* the caller vouches for the workspace: its first 512 bytes were zero when it was allocated  */
                                  /* and nothing but irec_beam_encode has written to it since.  Every call stamps the key of  */
                                  /* each proposal table it builds (seed, S, D, table window, table kind, offset) into the    */
                                  /* workspace head; with this flag a later call on the SAME workspace whose key matches the  */
                                  /* stamp -- checked on the device, so also inside a replayed HIP graph -- keeps the table   */
                                  /* instead of rebuilding it (the 24 residual blocks of an image share seed, S and dims:     */
                                  /* beam_search_coder.py:38-43, resnet_vae.py:822-824).  Same outputs, bit for bit.          */
#define IREC_FLAG_MARGINS 524288   /* the call reports its top-B margins: irec_beam_encode_ex with out_margin (and only that entry point) takes it.  The    */
                                  /* flag is part of the params because it sizes the workspace (irec_encode_workspace_bytes) and picks the kernels     */
                                  /* (irec_encode_plan): a margin build of the team encoder where one exists, the generic kernel otherwise; no block   */
                                  /* is shared between workgroups or teams.  Indices, K and samples are the plain call's, bit for bit.                 */
/* (diagnostic flag bits -- pinned kernel shapes, A/B switches, test hooks -- and the unit-test entry points: csrc/irec_internal.h) */
#define IREC_TABLE_STEPS_DEFAULT 32
#define IREC_TABLE_STEPS_MAX 4096
#define IREC_TABLE_BYTES_MAX (64u << 20)
#define IREC_TABLE_STEPS_FLOOR 8            /* ... but the byte bound never cuts the window below 8 steps (one step of S = 8103, */
#define IREC_TABLE_BYTES_HARD (1u << 30)    /* the reference's largest, is 19 MB for 1000 + 192 dims) unless those exceed 1 GB   */
#define IREC_SLAB_BYTES_MAX (16ull << 30)   /* scratch slabs of a call whose blocks exceed 1024 dims: one per resident team, but no more than this  */
                                            /* holds (a 301 056-dim block needs 55 MB of slab: 290 teams instead of 768 code such a call)         */
#define IREC_TABLE_BYTES_BIG (4ull << 30)   /* the bound of calls whose blocks exceed 1024 dims (block_size = None on a whole tensor:  */
                                            /* K grows with the dims -- an 8192-dim block has ~60 partitions of 590 KB of rows each)   */

/* What irec_beam_encode does for a given call: filled by irec_encode_plan from the settled plan the launch itself runs from. */
typedef struct {
  char kernel[64];         /* block kernel, e.g. "encode_team_kernel<20,2,1>"                                   */
  char table_kernel[32];   /* who builds the proposal tables: "prep_kernel (copy bits)" / "prep_kernel (plain rows)" -- the call's one */
                           /* preparation launch (books, exchange granules, row costs, tables) -- or "" (Philox fused in the block kernel) */
  int32_t grid;            /* workgroups of the block kernel                                                    */
  int32_t waves_per_wg;
  int32_t teams_per_wg;    /* independent teams inside a workgroup (1 for the one-workgroup-per-block encoders) */
  int32_t lds_bytes;       /* dynamic LDS of one workgroup                                                      */
  int32_t table_steps;     /* partitions the proposal tables cover (0 = no tables)                              */
  int32_t n_tables;
  int32_t split;           /* workgroups that share one block (split encoder of calls of < 64 blocks), or teams that share each */
                           /* row beyond one per CU (team encoder, calls of one to 1.5 blocks per CU), or the teams of a gang  */
                           /* (chunked encoder, calls of <= 384 blocks of more than 1024 dims: chunk owners x sample stripes,  */
                           /* kernel "...,gang>"); 0 = nothing is shared                                                       */
  int32_t n_cu;            /* compute units of the context's device                                             */
  int32_t clock_mhz;       /* its maximum engine clock                                                          */
  int32_t split_beams;     /* split encoder: 1 = the workgroups of a block share its beams (each owns <= 2 beam slots,  */
                           /* scores every sample for them, forms only its own new beams), 0 = they share its samples  */
  int64_t table_bytes;     /* proposal tables inside the workspace                                              */
  int64_t workspace_bytes; /* = irec_encode_workspace_bytes()                                                   */
} irec_plan_info;

typedef struct irec_context irec_context;

/* ---- host-only helpers ---------------------------------------------------------------------------------- */
const char *irec_last_error(void);
const char *irec_version(void);

/* int(np.exp(kl_per_partition * extra_samples))  -- beam_search_coder.py:29 */
int32_t irec_n_samples(double kl_per_partition, double extra_samples);

/* len(indices) * np.log(n_samples)  -- BeamSearchCoder.get_codelength, beam_search_coder.py:150-151 (nats) */
double irec_codelength(int64_t n_indices, int32_t n_samples);

/* lut[k] = Normal(0,1).quantile(float32(k)/10007) for k = 1..10006, lut[0] = 0
 * -- the 10006 values dist.quantile can take in get_pseudo_random_sample, beam_search_coder.py:45-49. */
irec_status irec_build_lut(float *lut10007);

/* perm = tf.random.shuffle(tf.range(n)) after tf.random.set_seed(seed) -- Coder.split/merge, coder.py:62-64,111-113.
 * Host memory. */
irec_status irec_tf_shuffle_perm(int64_t seed, int64_t n, int64_t *perm);

/* ---- importance sampler (config 1 plumbing; the reference runs it on the CPU, and so does this: host memory) ---------
 * encode_gaussian_importance_sample (rec/coding/importance_sampling.py:9-79): standardise the target w.r.t. the coder,
 * draw n_samples = ceil(exp(coding_bits * log 2)) proposals x[s] ~ N(0,1)^n from the stream of tf.random.set_seed(seed);
 * tfd.Normal(0,1).sample(n_samples) (:37,50-53), weight them by w[s] = sum_d [log N(x; t', s') - log N(x; 0, 1)] (:57-58).
 *   alpha = inf : index = argmax_s w[s] (first one on ties, tf.argmax :64)
 *   1 <= alpha  : index = argmax_s alpha * w[s] + g[s], g = stateless_gumbel_sample([n_samples], seed + 1) (:67-71;
 *                 rec/coding/utils.py:9-12 puts a stateless NORMAL draw inside -log(-log(.)), so g is NaN for most s and
 *                 tf.argmax skips those: reproduced as written)
 *   alpha < 1   : error (:33-34)
 * Returns the index and p_scale * x[index] + p_loc (:73-76).  n = number of dims of the (flattened) distributions. */
irec_status irec_importance_encode(const float *t_loc, const float *t_scale, const float *p_loc, const float *p_scale,
                                   int64_t n, double coding_bits, double alpha, int64_t seed, int64_t *out_index,
                                   float *out_sample);
/* decode_gaussian_importance_sample (importance_sampling.py:82-103): sample `index` of the same stream. */
irec_status irec_importance_decode(const float *p_loc, const float *p_scale, int64_t n, int64_t index, int64_t seed,
                                   float *out_sample);
/* n_samples of the call above (float32 arithmetic as in importance_sampling.py:50), or -1 if it does not fit int32. */
int64_t irec_importance_n_samples(double coding_bits);
/* out[e] = element e of tf.random.uniform([n], 1, 10007, seed=seed, dtype=int32) after tf.random.set_seed(seed)
 * -- beam_search_coder.py:38-43.  Host memory; test hook for the in-kernel Philox stream. */
irec_status irec_philox_uniform_int(int64_t seed, int64_t n, int32_t *out);

/* ---- context ---------------------------------------------------------------------------------------------- */
/* Builds the constant tables (quantile LUT in discrete-log order, discrete-log table of Z_10007^*, power-law ratios
 * get_auxiliary_ratio, coder.py:16,218-220) and uploads them to HIP device `device`.
 * Fails with IREC_E_NO_DEVICE when there is no GPU: there is no CPU fallback. */
irec_status irec_create(int device, irec_context **out);
/* irec_create with the path's TF-dependent primitive supplied by the caller.
 *   lut10007  host float [10007], may be NULL (= irec_build_lut): lut10007[k] = the float32 that
 *             tfd.Normal(0, 1).quantile(float32(k) / 10007) returns in the CALLER's TensorFlow, k = 1..10006 (entry 0 is never
 *             indexed) -- the 10006 values `dist.quantile` can take at beam_search_coder.py:48-49 before the scale is applied.
 *             Every kernel of the context (encoders, decoders) reads its quantiles from this table and from nothing else.
 * Why: irec_build_lut restates TFP 0.9's float32 ndtri with a correctly rounded log; TensorFlow evaluates it over Eigen's
 * vectorised log, and a 1-ulp difference in one entry can move an emitted index.  A maintainer with a TF 2.1 machine dumps
 * the table once (scripts/make_tf_vectors.py writes it as `quantile` in tf_primitives.npz) and creates the context with it:
 * the stream then decodes on the TensorFlow side, no recompile.  (The other TF-dependent input, the tf.random.shuffle
 * permutation of Coder.split, is a caller argument already: `perm` of irec_beam_encode / irec_beam_decode.)
 * All entries 1..10006 must be finite (IREC_E_INVALID otherwise). */
irec_status irec_create_ex(int device, const float *lut10007, irec_context **out);
/* The context's caller-supplied tables in one (extensible) struct; zero-initialise it, every member is optional.
 *   lut10007       as irec_create_ex.
 *   aux_ratios     host float [n_aux_ratios]: the FITTED auxiliary-variance ratios of a coder constructed with
 *                  extrapolate_auxiliary_ratios=False -- the values of its `aux_variable_variance_ratios` variable, which
 *                  GaussianCoder.get_auxiliary_ratio(index) returns in place of the power law (coder.py:203-231; the SGD fitter that
 *                  produces them, coder.py:233-410, is irec_fit_aux_ratios below).  Every entry must lie in (0, 1].
 *                  A block whose K = ceil(KL / Omega) exceeds n_aux_ratios is NOT coded (out_K = K is still written, as for K > max_K):
 *                  the reference raises "KL divergence higher than auxiliary variables can account for" there (coder.py:222-229), and so
 *                  does the Python mirror.  The decoder treats such a row as not decodable.  irec_max_partitions(ctx) tells the bound. */
typedef struct {
  const float *lut10007;
  const float *aux_ratios;
  int32_t n_aux_ratios;
} irec_tables;
irec_status irec_create_with(int device, const irec_tables *tables, irec_context **out);
/* Partitions the context's auxiliary ratios cover: IREC_MAX_PARTITIONS (power law) or n_aux_ratios. */
int32_t irec_max_partitions(const irec_context *ctx);
void irec_destroy(irec_context *ctx);

/* Bytes of device scratch irec_beam_encode needs for blocks of at most max_dim dims and max_K partitions. */
size_t irec_encode_workspace_bytes(const irec_context *ctx, const irec_params *p, int32_t max_dim, int32_t max_K);

/* The same for ONE call of n_blocks blocks (round 6).  Differs from the bound above only for blocks of more than 1024 dims (block_size = None,
 * 2048, ...): their scratch slab is (6 + 2 B) x dims x 4 bytes per team -- 55 MB at 301 056 dims -- and the bound above reserves one per team slot
 * of the device (at most IREC_SLAB_BYTES_MAX = 16 GB, plus up to IREC_TABLE_BYTES_BIG = 4 GB of proposal tables and 1 GB of gang exchange),
 * whereas a call uses one per team it launches: n_blocks x (teams per gang).  irec_beam_encode takes either size, or any size in between (it launches
 * no more teams than the workspace has slabs; same results). */
size_t irec_encode_workspace_bytes_for(const irec_context *ctx, const irec_params *p, int64_t n_blocks, int32_t max_dim, int32_t max_K);

/* The kernels, grid and scratch irec_beam_encode(ctx, p, n_blocks, ..., max_block_dim, ..., max_K, ...) launches.
 * Host only, no device work; bench.py reports the kernel it measured from this instead of a string literal. */
irec_status irec_encode_plan(const irec_context *ctx, const irec_params *p, int64_t n_blocks, int32_t max_block_dim,
                             int32_t max_K, irec_plan_info *out);

/* ---- device entry points ---------------------------------------------------------------------------------- */

/* total_kl and num_aux_variables of every block -- beam_search_coder.py:57-59.
 *   out_kl [n_blocks] float32 (may be NULL), out_K [n_blocks] int32.  Device pointers. */
irec_status irec_block_kl(irec_context *ctx, const irec_params *p, int64_t n_blocks, const int64_t *block_base,
                          const int32_t *block_pos, const int32_t *block_dim, const int32_t *perm,
                          const float *q_loc, const float *q_scale, const float *p_loc, const float *p_scale,
                          float *out_kl, int32_t *out_K, void *hip_stream);

/* BeamSearchCoder.encode_block on n_blocks independent blocks -- beam_search_coder.py:53-122, driven the way
 * GaussianCoder.encode drives it (same seed for every block, coder.py:444-449).
 *   max_block_dim                   upper bound of block_dim[] (host knows it: block_size); a block with more dims
 *                                   is not coded and gets out_K = -1
 *   out_K       [n_blocks]          K of each block.  K > max_K means "not coded: retry with a larger max_K"; -1: the block's
 *                                   dim is not covered by max_block_dim / table_dims; -2: the block was shared between workgroups or
 *                                   teams and its partners were not all resident within 100 ms (a co-tenant on the device, two
 *                                   cooperating calls in flight): call again, or with IREC_FLAG_NO_SPLIT.
 *   out_indices [n_blocks, max_K]   idx[t], t < K: the sample index chosen at iteration t (rest untouched)
 *   out_sample  flat, same indexing as the inputs: beams[0] + p.loc, merged
 *   workspace   device scratch of at least irec_encode_workspace_bytes() -- or irec_encode_workspace_bytes_for(n_blocks) -- bytes, 256-byte aligned
 * All pointers except p are device pointers. */
irec_status irec_beam_encode(irec_context *ctx, const irec_params *p, int64_t n_blocks, const int64_t *block_base,
                             const int32_t *block_pos, const int32_t *block_dim, int32_t max_block_dim,
                             const int32_t *perm, const float *q_loc, const float *q_scale, const float *p_loc,
                             const float *p_scale, int64_t seed, int32_t max_K, int32_t *out_K, int32_t *out_indices,
                             float *out_sample, void *workspace, size_t workspace_bytes, void *hip_stream);

/* irec_beam_encode that also says HOW CLOSE every block's selections were (round 5) -- the top-B step of beam_search_coder.py:85-89
 * (`tf.argsort(..., direction='DESCENDING')[:n_beams]`) decides the emitted indices through two comparisons only: which candidates
 * make the top-B SET of every step but the last, and which candidate WINS the last step (beams[0], :118-122).  Another float32
 * summation order of the same terms -- TensorFlow's reduce_sum (:84) -- can move an index only where those
 * comparisons are closer than the two orders disagree, so the margins measure the encoder-side exposure of index parity.
 *   out_margin [n_blocks][4] float32, device pointer; needs IREC_FLAG_MARGINS in p->flags (NULL without it: plain irec_beam_encode):
 *     [0] min over the steps t < K - 1 that reject a candidate of  score(rank Bnew - 1) - score(rank Bnew), Bnew = min(B, S * Bcur):
 *         the gap between the last candidate kept and the best one rejected; +inf when there is no such step (K <= 1)
 *     [1] |score(rank Bnew - 1)| at that step (scale of the sum the gap is a difference of)
 *     [2] score(rank 0) - score(rank 1) at the last step (+inf: a single candidate)        [3] |score(rank 0)| at the last step
 *   Scores are the float32 values the selection ranks, differences are float32 subtractions: the oracle's traced
 *   scores give the same four numbers bit for bit.  A block that is not coded (K = 0, K > max_K, K < 0) reports {+inf, 0, +inf, 0}.
 *   Decoding needs none of this: decode_block never compares scores (beam_search_coder.py:124-148). */
irec_status irec_beam_encode_ex(irec_context *ctx, const irec_params *p, int64_t n_blocks, const int64_t *block_base,
                                const int32_t *block_pos, const int32_t *block_dim, int32_t max_block_dim,
                                const int32_t *perm, const float *q_loc, const float *q_scale, const float *p_loc,
                                const float *p_scale, int64_t seed, int32_t max_K, int32_t *out_K, int32_t *out_indices,
                                float *out_sample, float *out_margin, void *workspace, size_t workspace_bytes, void *hip_stream);

/* BeamSearchCoder.decode_block on n_blocks blocks -- beam_search_coder.py:124-148 (GaussianCoder.decode, coder.py:459-491).
 *   K [n_blocks], indices [n_blocks, max_K] in ENCODER order (idx[t] = choice at iteration t).  A row with K < 0 or
 *   K > max_K (what the encoder leaves for a block it did not code), or one that holds an index outside [0, n_samples) (a
 *   damaged or foreign stream; the reference fails in tf.gather), is not decodable: the block's elements are returned as
 *   p_loc -- by every decode entry point, and no table row outside the call's tables is ever addressed.  So is a block whose
 *   dim exceeds the call's bound (max_block_dim, or the largest listed table dim when there is none). */
irec_status irec_beam_decode(irec_context *ctx, const irec_params *p, int64_t n_blocks, const int64_t *block_base,
                             const int32_t *block_pos, const int32_t *block_dim, const int32_t *perm,
                             const float *p_loc, const float *p_scale, int64_t seed, int32_t max_K, const int32_t *K,
                             const int32_t *indices, float *out_sample, void *hip_stream);

/* The same decode with caller-provided scratch (irec_decode_workspace_bytes(), 256-byte aligned; may be NULL / 0): with
 * p->table_dims set the shared-seed draw of the call is evaluated once into per-call proposal tables (every block of one dim
 * count reads its rows from the same S rows per step, beam_search_coder.py:38-43,141-146) instead of once per block -- same
 * outputs, bit for bit.  max_block_dim: upper bound of block_dim[] (>= every listed table dim).  A block whose dim exceeds it
 * is not decoded.  With table_dims set, irec_beam_decode above takes the same kernel without the tables. */
size_t irec_decode_workspace_bytes(const irec_context *ctx, const irec_params *p, int32_t max_K);
irec_status irec_beam_decode_ws(irec_context *ctx, const irec_params *p, int64_t n_blocks, const int64_t *block_base,
                                const int32_t *block_pos, const int32_t *block_dim, int32_t max_block_dim,
                                const int32_t *perm, const float *p_loc, const float *p_scale, int64_t seed, int32_t max_K,
                                const int32_t *K, const int32_t *indices, float *out_sample, void *workspace,
                                size_t workspace_bytes, void *hip_stream);

/* GaussianCoder.decode (coder.py:459-491) on n_tensors whole tensors of tensor_dims dims lying back to back in p_loc /
 * p_scale / out_sample, cut the way Coder.split cuts them (coder.py:69-83): block j of a tensor = shuffled positions
 * [j * block_size, min((j + 1) * block_size, tensor_dims)) through perm [tensor_dims] (NULL: no shuffle).  One workgroup
 * decodes all blocks of a tensor with sigma_p / mu_p / the samples staged in LDS, so split and merge touch global memory
 * in natural order only (the element-wise gathers of irec_beam_decode cost three times the arithmetic).
 *   K [n_tensors * bpt], indices [n_tensors * bpt, max_K], bpt = ceil(tensor_dims / block_size): row of block j of tensor i
 *   is block_row[i * bpt + j] (device int32; NULL: i * bpt + j).  p->table_dims is ignored (derived from the sizes).
 * Same outputs as irec_beam_decode, bit for bit.  Applies when irec_decode_tensors_supported() (tensors that fit the LDS);
 * workspace as for irec_beam_decode_ws (irec_decode_workspace_bytes with table_dims = {block_size, last block's dim}). */
int32_t irec_decode_tensors_supported(const irec_params *p, int32_t tensor_dims, int32_t block_size);
irec_status irec_beam_decode_tensors(irec_context *ctx, const irec_params *p, int64_t n_tensors, int32_t tensor_dims,
                                     int32_t block_size, const int32_t *block_row, const int32_t *perm, const float *p_loc,
                                     const float *p_scale, int64_t seed, int32_t max_K, const int32_t *K,
                                     const int32_t *indices, float *out_sample, void *workspace, size_t workspace_bytes,
                                     void *hip_stream);

/* ---- the sequential importance coder: GaussianCoder(sampler=ImportanceSampler(coding_bits, alpha)), 1 <= alpha <= inf ------
 * GaussianCoder.encode_block / decode_block (rec/coding/coder.py:493-584) driven the way GaussianCoder.encode / decode drive them
 * (coder.py:412-491: the same seed for every block): per block K = ceil(KL / Omega) serial steps -- K - 1 auxiliary variables
 * (ratio get_auxiliary_ratio(i), i = K-1 .. 1), then the block's sample -- each one encode_gaussian_importance_sample
 * (importance_sampling.py:9-79) with seed + step, followed by the conditional update of target and coder (coder.py:157-171).
 * A block emits max(K, 1) indices (a zero-KL block one, coder.py:548-557).  Arithmetic: DESIGN.md §3.
 * alpha = inf (the reference's default): a step takes the first greatest importance weight -- irec_gc_importance_encode / _ws.
 * 1 <= alpha < inf: the Gumbel-max over alpha * w + g (importance_sampling.py:67-72) -- irec_gc_importance_encode_gumbel with the
 * perturbations g as one more table.  The decoder never looks at alpha: irec_gc_importance_decode serves both.
 *
 * The standard-normal proposals of step j are tf.random.normal([S, 1, D]) after tf.random.set_seed(seed + j): they depend on
 * (seed + j, S, D) only, so every block of D dims reads the same S x D numbers at step j.  They pass through libm on the host
 * (and through Eigen in TensorFlow), so they are DATA the kernels read, built by the caller -- like lut10007:
 *   out[(j * dim + d) * S_pad + s] = element s * dim + d of the stream of seed + j,  j < steps, d < dim, s < n_samples,
 *   S_pad = n_samples rounded up to IREC_NORMAL_TABLE_PAD (sample index fastest; the padding is zero).
 * irec_normal_table_floats: floats of one table, or 0 (text in irec_last_error) for sizes out of range or a table of more than
 * IREC_TABLE_BYTES_HARD bytes.  irec_normal_table_build: host memory, n_threads host threads (0: one per core, at most 16). */
#define IREC_NORMAL_TABLE_PAD 16
size_t irec_normal_table_floats(int32_t n_samples, int32_t dim, int32_t steps);
irec_status irec_normal_table_build(int64_t seed, int32_t n_samples, int32_t dim, int32_t steps, float *out, int32_t n_threads);

/* The tables of one call, on the device: table[i] serves the blocks of dim[i] dims (unused slots: NULL / 0), all built with the
 * call's seed, n_samples = ceil(exp(coding_bits * log 2)) (irec_importance_n_samples) and `steps`. */
typedef struct {
  const float *table[4];
  int32_t dim[4];
  int32_t n_samples;
  int32_t steps;
} irec_normal_tables;

/* Encode n_blocks blocks (layout arguments as irec_beam_encode; blocks of at most 1024 dims -- wider ones: the _ws entry below).
 * Asynchronous, no workspace.
 *   max_K       index slots per row, 1 <= max_K <= tables->steps
 *   out_K       [n_blocks] K = ceil(KL / kl_per_partition) of each block (the K of irec_block_kl).  K > max_K: not coded, call
 *               again with a longer window; K > irec_max_partitions(ctx) (fitted ratios): not coded; -1: no table of the block's
 *               dim, or (this entry only) more than 1024 dims
 *   out_indices [n_blocks, max_K]: idx[t], t < max(K, 1), the sample chosen at step t (rest untouched)
 *   out_sample  flat, indexed as the inputs (merged)
 * Hand the blocks over longest first (by K): a workgroup codes one block at a time. */
irec_status irec_gc_importance_encode(irec_context *ctx, int64_t n_blocks, const int64_t *block_base, const int32_t *block_pos,
                                      const int32_t *block_dim, const int32_t *perm, const float *q_loc, const float *q_scale,
                                      const float *p_loc, const float *p_scale, const irec_normal_tables *tables,
                                      float kl_per_partition, int32_t max_K, int32_t *out_K, int32_t *out_indices,
                                      float *out_sample, void *hip_stream);
/* The same for blocks of ANY dim: the remaining limit is the size of the tables (IREC_TABLE_BYTES_HARD, IREC_TABLE_STEPS_MAX).
 * The call's largest block is the largest tables->dim[i] that has a table.  At most 1024 dims: dispatched exactly as
 * irec_gc_importance_encode -- same kernel, same launch, the workspace is ignored (it may be NULL).  More: one kernel codes every
 * block of the call, narrow ones included (the same bits: DESIGN.md §3), and keeps a block's state in a slab of the workspace,
 * four float arrays of max_block_dim rounded up to 1024 per workgroup.
 * GRID RULE: min(n_blocks, compute units of the context) workgroups of 1024 lanes, each coding one block at a time;
 * irec_gc_encode_workspace_bytes = that many slabs (rounded up to 256 bytes), 0 when max_block_dim <= 1024 or n_blocks == 0.
 * A workspace that is NULL, not 256-byte aligned or smaller than that: IREC_E_WORKSPACE with the needed size in irec_last_error;
 * nothing is launched and the outputs are untouched. */
size_t irec_gc_encode_workspace_bytes(irec_context *ctx, int64_t n_blocks, int32_t max_block_dim);
irec_status irec_gc_importance_encode_ws(irec_context *ctx, int64_t n_blocks, const int64_t *block_base, const int32_t *block_pos,
                                         const int32_t *block_dim, const int32_t *perm, const float *q_loc, const float *q_scale,
                                         const float *p_loc, const float *p_scale, const irec_normal_tables *tables,
                                         float kl_per_partition, int32_t max_K, int32_t *out_K, int32_t *out_indices,
                                         float *out_sample, void *workspace, size_t workspace_bytes, void *hip_stream);
/* ---- finite alpha: the Gumbel-max branch (importance_sampling.py:67-72) ----
 * The perturbations of step j are g = stateless_gumbel_sample([S], seed + j + 1) = -logf(-logf(z)), z = tf.random.stateless_normal([S],
 * [seed + j + 1, seed + j + 2]) (rec/coding/utils.py:9-12: a NORMAL draw inside the double log, so g is NaN for about two samples in
 * three -- reproduced as written).  They pass through libm on the host, so they are DATA the kernels read, like the normal tables, and
 * irec_importance_encode evaluates the same function:
 *   out[j * S_pad + s] = g[s] of step j,  j < steps, s < n_samples, S_pad as above (the padding is zero, and no lane reads it).
 * irec_gumbel_table_floats: floats of the table, or 0 (text in irec_last_error) for sizes out of range.  irec_gumbel_table_build: host
 * memory, n_threads host threads (0: one per core, at most 16). */
size_t irec_gumbel_table_floats(int32_t n_samples, int32_t steps);
irec_status irec_gumbel_table_build(int64_t seed, int32_t n_samples, int32_t steps, float *out, int32_t n_threads);
typedef struct {
  const float *table;   /* device: irec_gumbel_table_build(seed, n_samples, steps) -- or any numbers of the caller's: they are data */
  int32_t n_samples;
  int32_t steps;
  float alpha;
} irec_gumbel_table;
/* irec_gc_importance_encode_ws over v[s] = float32(alpha) * w[s] + g[step][s] (one float32 multiply, then one float32 add): the index of
 * a step is the first s with the greatest v[s], the accumulator starts at (0, -FLT_MAX) and moves on a strict ">" -- a NaN is never
 * chosen, +inf can win, -inf never does.  The conditional update and the emitted sample use x[index] as at alpha = inf.
 *   gumbel == NULL  irec_gc_importance_encode_ws, bit for bit (the same kernels)
 *   otherwise       gumbel->n_samples and ->steps must equal tables->n_samples and ->steps, and alpha must be finite and >= 1:
 *                   IREC_E_INVALID otherwise, nothing is launched and the outputs are untouched
 * Grid rule, workspace and every other argument: as irec_gc_importance_encode_ws. */
irec_status irec_gc_importance_encode_gumbel(irec_context *ctx, int64_t n_blocks, const int64_t *block_base, const int32_t *block_pos,
                                             const int32_t *block_dim, const int32_t *perm, const float *q_loc, const float *q_scale,
                                             const float *p_loc, const float *p_scale, const irec_normal_tables *tables,
                                             float kl_per_partition, int32_t max_K, int32_t *out_K, int32_t *out_indices,
                                             float *out_sample, void *workspace, size_t workspace_bytes,
                                             const irec_gumbel_table *gumbel, void *hip_stream);
/* Decode: K [n_blocks], indices [n_blocks, max_K] in encoder order, max(K, 1) entries per row.  A row with K < 0, K > max_K,
 * K > irec_max_partitions(ctx), an index outside [0, n_samples) or a dim without a table decodes to p_loc, as irec_beam_decode
 * promises; any block dim with a table is served. */
irec_status irec_gc_importance_decode(irec_context *ctx, int64_t n_blocks, const int64_t *block_base, const int32_t *block_pos,
                                      const int32_t *block_dim, const int32_t *perm, const float *p_loc, const float *p_scale,
                                      const irec_normal_tables *tables, int32_t max_K, const int32_t *K, const int32_t *indices,
                                      float *out_sample, void *hip_stream);

/* ---- the fitter of the auxiliary-variance ratios: GaussianCoder.update_block_auxiliary_variance_ratios (coder.py:266-410) ----------
 * For ratio = M .. 2 (M = the largest 1 + floor(KL / Omega) of the rows, coder.py:284): an SGD over the rows with at least `ratio`
 * partitions finds the variance ratio whose auxiliary variable carries Omega nats and leaves Omega * (ratio - 1), the result is
 * averaged into ratios[ratio - 1] (coder.py:385-389), and the rows are conditioned on a draw of that auxiliary variable
 * (coder.py:390-408).  Arithmetic: DESIGN.md §3 "ratio fit" -- float64 over det_log / det_exp, canonical reduction trees; the device
 * entry point and the host twin give the same bits.
 *   q_loc .. p_scale  [n_rows, dim] float32, row-major; not modified (the conditional statistics live in the workspace)
 *   normal_table      irec_normal_table_build(seed, n_samples = n_rows, dim, steps = table_steps): the draw of row n, dim d at fit step j
 *                     (ratio = M - j) is element n * dim + d of tf.random.normal after tf.random.set_seed(seed + j).  The reference draws
 *                     from TensorFlow's unseeded global generator there (aux_target.sample(), coder.py:393); here the fit is seeded.
 *                     table_steps >= M - 1 (irec_fit_partitions tells M beforehand); may be NULL when M <= 1.
 *   ratios, average_counts  HOST float32 [capacity], in/out: the coder's `aux_variable_variance_ratios` and `average_counts`
 *                     (initially {1.} each, coder.py:203-212); *length entries are valid on entry, max(*length, M) on return
 *                     (grown with zeros, coder.py:289-302)
 *   out_iters         HOST int32 [M - 1]: SGD iterations of every fit step
 *   workspace         irec_fit_workspace_bytes(n_rows, dim) bytes, 256-byte aligned: device memory for irec_fit_aux_ratios / irec_fit_partitions,
 *                     host memory for irec_fit_aux_ratios_host
 * irec_fit_aux_ratios enqueues one launch per SGD iteration in chunks and reads a `done` word between chunks: it SYNCHRONISES the stream
 * and returns when the fit is over.  No kernel waits for another workgroup.  Two fits on two streams (two workspaces) may run at once.
 * An infinite or NaN KL, M > IREC_MAX_PARTITIONS, M > capacity or a table of fewer than M - 1 steps: IREC_E_INVALID, nothing fitted.
 * The host twin needs no GPU and no context; n_threads host threads over rows (0: one per core, at most 16). */
typedef struct {
  float kl_per_partition;      /* Omega (float32, coder.py:192) */
  double relative_tolerance;   /* stop when |previous loss - loss| < this (coder.py:373) */
  double learning_rate;        /* SGD step (coder.py:335) */
  int32_t max_iters;           /* iterations per fit step, at most (coder.py:340); >= 1 */
} irec_fit_params;
size_t irec_fit_workspace_bytes(int64_t n_rows, int32_t dim);
/* out_kl [n_rows] float32 canonical KL of every row, out_num [n_rows] = 1 + floor(kl / Omega) in float32 (coder.py:282-284): HOST memory. */
irec_status irec_fit_partitions(irec_context *ctx, float kl_per_partition, int64_t n_rows, int32_t dim, const float *q_loc,
                                const float *q_scale, const float *p_loc, const float *p_scale, float *out_kl, int32_t *out_num,
                                void *workspace, size_t workspace_bytes, void *hip_stream);
irec_status irec_fit_partitions_host(float kl_per_partition, int64_t n_rows, int32_t dim, const float *q_loc, const float *q_scale,
                                     const float *p_loc, const float *p_scale, float *out_kl, int32_t *out_num, int32_t n_threads);
irec_status irec_fit_aux_ratios(irec_context *ctx, const irec_fit_params *p, int64_t n_rows, int32_t dim, const float *q_loc,
                                const float *q_scale, const float *p_loc, const float *p_scale, const float *normal_table,
                                int32_t table_steps, float *ratios, float *average_counts, int32_t capacity, int32_t *length,
                                int32_t *out_iters, void *workspace, size_t workspace_bytes, void *hip_stream);
irec_status irec_fit_aux_ratios_host(const irec_fit_params *p, int64_t n_rows, int32_t dim, const float *q_loc, const float *q_scale,
                                     const float *p_loc, const float *p_scale, const float *normal_table, int32_t table_steps,
                                     float *ratios, float *average_counts, int32_t capacity, int32_t *length, int32_t *out_iters,
                                     void *workspace, size_t workspace_bytes, int32_t n_threads);

/* ---- .rec wire format: entropy coder of the index streams (host memory; the reference's is CPU Cython too) ------------ */
const char *irec_io_last_error(void);
/* ArithmeticCoder(counts, precision).encode(message) -- rec/io/entropy_coding.pyx:51-121.  out_bits: one ASCII '0'/'1'
 * per code bit; *n_bits = code length (also when it exceeds cap, in which case an error is returned). */
irec_status irec_ac_encode(const int64_t *counts, int32_t n_symbols, const int64_t *message, int64_t n_message,
                           int32_t precision, uint8_t *out_bits, int64_t cap, int64_t *n_bits);
/* ArithmeticCoder.decode_fast(code) -- rec/io/entropy_coding.pyx:213-302 (symbol lookup of data_structures.py:186-213
 * by binary search).  Decodes up to and including the terminator symbol 0. */
irec_status irec_ac_decode(const int64_t *counts, int32_t n_symbols, const uint8_t *bits, int64_t n_bits,
                           int32_t precision, int64_t *out_message, int64_t cap, int64_t *n_message);
/* int('1' + code, 2).to_bytes(ceil((len + 1) / 8), 'big') -- rec/io/utils.py:66-72,100-106.  Returns bytes written or -1. */
int64_t irec_rec_pack_bits(const uint8_t *bits, int64_t n_bits, uint8_t *out_bytes, int64_t cap);
/* bin(int.from_bytes(bytes, 'big'))[3:] -- rec/io/utils.py:158-170.  Returns code bits written or -1. */
int64_t irec_rec_unpack_bits(const uint8_t *bytes, int64_t n_bytes, uint8_t *out_bits, int64_t cap);

/* Whole .rec files with the default symbol models, one call each (the per-stream Python glue of the reference, utils.py:55-106 and
 * :150-216, costs more host time per image than the GPU takes to code it).
 * write_compressed_code(file_path, seed, image_shape, block_size, block_indices, max_index) -- rec/io/utils.py:7-106:
 *   blocks_per_res [R]; K [sum blocks_per_res] partitions of every coded block, residual block after residual block;
 *   indices [sum K] their sample indices back to back.  Returns the file's byte count (also when > cap: call again), -1 on error. */
int64_t irec_rec_encode_file(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                             uint32_t channels, int32_t n_res_blocks, const int32_t *blocks_per_res, const int32_t *K,
                             const int32_t *indices, uint8_t *out, int64_t cap);
/* read_compressed_code -- rec/io/utils.py:109-216.  header_out[9] = seed, block_size, max_index, height, width, channels,
 * uses_count_file, uses_index_file, R; sizes_out[3] = R, coded blocks, indices.  IREC_E_WORKSPACE (sizes filled) when an
 * output array is null or short. */
irec_status irec_rec_decode_file(const uint8_t *bytes, int64_t n_bytes, uint32_t *header_out, int64_t *sizes_out,
                                 int32_t *blocks_per_res, int64_t cap_res, int32_t *K, int64_t cap_blocks, int32_t *indices,
                                 int64_t cap_indices);

/* Many containers at once (host threads; n_threads = 0: one per core, at most 32).  A batched model pass hands over ONE packed
 * read-back for all its images -- K [n_images][R][bpt], idx [n_images][R][bpt][max_K] (first K entries of a row count), R
 * residual blocks of bpt coded blocks each -- instead of nested per-image lists (the per-image loop of
 * compression_performance.py:350-375: write_compressed_code, then read_compressed_code and compare).
 * irec_rec_encode_files: the n_images files back to back in out, offsets [n_images + 1]; every file byte for byte what
 * irec_rec_encode_file gives for that image.  Returns the total byte count (also when > cap: call again), -1 on error.
 * irec_rec_decode_files: the inverse, rows zero-filled past K; headers [n_images][9] as irec_rec_decode_file's header_out. */
int64_t irec_rec_encode_files(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                              uint32_t channels, int32_t n_images, int32_t n_res_blocks, int32_t blocks_per_res, int32_t max_K,
                              const int32_t *K, const int32_t *idx, uint8_t *out, int64_t cap, int64_t *offsets, int32_t n_threads);
irec_status irec_rec_decode_files(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                  int32_t blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K, int32_t *idx,
                                  int32_t n_threads);
/* The same two calls for files whose residual blocks differ in size ("ragged": a two-level model codes 13 blocks at one level and 302
 * at the other).  blocks_per_res [R], every entry >= 1; first[r] = sum of the entries before r, T = first[R]; block j of residual block
 * r of image i is row i T + first[r] + j of K [n_images][T] and idx [n_images][T][max_K].  Bytes, return values and errors as above:
 * every file is what irec_rec_encode_file gives for that image, the reader's outputs are what irec_rec_decode_file gives, rows
 * zero-filled past K, and a file whose R or any block count differs from the call's fails the call naming the image. */
int64_t irec_rec_encode_files_ragged(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                     uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                     int32_t max_K, const int32_t *K /*[n][T]*/, const int32_t *idx /*[n][T][max_K]*/, uint8_t *out,
                                     int64_t cap, int64_t *offsets, int32_t n_threads);
irec_status irec_rec_decode_files_ragged(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                         const int32_t *blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K /*[n][T]*/,
                                         int32_t *idx /*[n][T][max_K]*/, int32_t n_threads);

/* The same two calls on the device (csrc/irec_rec.hip over csrc/irec_rec_core.h): the files of a batch built from, and read into,
 * device memory, one lane per stream, so that no index crosses to the host between a batch and its bytes.  Every pointer but
 * `workspace`'s size is a device pointer.  Asynchronous on hip_stream like every device entry point here: no allocation, no
 * synchronisation, no copy to the host inside; argument errors the host can see return IREC_E_INVALID.  Default symbol models only.
 * irec_rec_encode_files_device: block b = (i R + r) bpt + j has its count at K[b k_stride] and its row at idx[b idx_stride + t] --
 *   the packed arrays (k_stride 1, idx_stride max_K) or one joined [rows][1 + width] tensor (K in column 0, both strides
 *   1 + width).  offsets [n_images + 1] and status [n_images] are always written; a file with a nonzero status has no bytes.
 *   The bytes are written only if offsets[n_images] <= cap (else nothing at all: call again with that much room).
 * irec_rec_decode_files_device: headers [n][9], K [n][R][bpt], idx [n][R][bpt][max_K] as irec_rec_decode_files gives them; an image
 *   with a nonzero status has all three zeroed, and no read leaves its [offsets[i], offsets[i + 1]). */
typedef enum {
  IREC_REC_OK = 0,
  IREC_REC_E_K_RANGE = 1,           /* encode: a partition count outside [0, max_K]                                       */
  IREC_REC_E_INDEX_RANGE = 2,       /* encode: an index outside [0, max_index)                                            */
  IREC_REC_E_MODEL_RANGE = 3,       /* encode: the model's total exceeds 2^30 (max_index above ~1.07 million)             */
  IREC_REC_E_TRUNCATED_HEADER = 4,  /* decode: fewer bytes than the static or the dynamic header                          */
  IREC_REC_E_COUNT_FILES = 5,       /* decode: the file uses empirical count tables                                       */
  IREC_REC_E_MAX_INDEX = 6,         /* decode: max_index outside [1, 2^24]                                                */
  IREC_REC_E_BLOCK_COUNTS = 7,      /* decode: max_part above IREC_MAX_PARTITIONS, or more blocks than the count stream holds */
  IREC_REC_E_TRUNCATED_STREAMS = 8, /* decode: a stream ends past the file                                                */
  IREC_REC_E_COUNT_MARKER = 9,      /* decode: a count stream without its marker bit                                      */
  IREC_REC_E_COUNT_CORRUPT = 10,    /* decode: a count stream with target < 0 or width <= 0                               */
  IREC_REC_E_COUNT_BUDGET = 11,     /* decode: a count stream whose renormalisation budget ran out (no terminator)        */
  IREC_REC_E_INDEX_MODEL = 12,      /* decode: the header's max_index gives a model total above 2^30                      */
  IREC_REC_E_INDEX_MARKER = 13,     /* decode: an index stream without its marker bit                                     */
  IREC_REC_E_INDEX_CORRUPT = 14,    /* decode: an index stream with target < 0 or width <= 0                              */
  IREC_REC_E_INDEX_BUDGET = 15,     /* decode: an index stream whose renormalisation budget ran out (no terminator)       */
  IREC_REC_E_MISMATCH = 16,         /* decode: counts or indices do not match the header (also: more values than allowed) */
  IREC_REC_E_STRUCTURE = 17,        /* decode: not n_res_blocks residual blocks of the call's blocks_per_res blocks        */
  IREC_REC_E_MAX_K = 18,            /* decode: a block with more partitions than max_K                                    */
  IREC_REC_E_TABLE = 19,            /* a symbol table whose entries cannot be coded under (the *_tables entry points only) */
  IREC_REC_E_SEG_MAGIC = 20,        /* decode, segmented: not the magic "IRSG", version 1, reserved 0                       */
  IREC_REC_E_SEG_DIRECTORY = 21,    /* decode, segmented: header + directory + the streams it lists are not the file's length */
  IREC_REC_E_SEG_BLOCKS = 22        /* decode, segmented: segment_blocks is 0 or not the call's                             */
} irec_rec_status;
size_t irec_rec_device_workspace_bytes(int32_t n_images, int32_t n_res_blocks);
irec_status irec_rec_encode_files_device(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                         uint32_t channels, int32_t n_images, int32_t n_res_blocks, int32_t blocks_per_res, int32_t max_K,
                                         const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                         uint8_t *out, int64_t cap, int64_t *offsets /*[n_images + 1]*/, int32_t *status /*[n_images]*/,
                                         void *workspace, size_t workspace_bytes, void *hip_stream);
irec_status irec_rec_decode_files_device(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                         int32_t blocks_per_res, int32_t max_K, uint32_t *headers /*[n][9]*/, int32_t *K, int32_t *idx,
                                         int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream);
/* The ragged forms of the two device calls: the layout of irec_rec_encode_files_ragged (row i T + first[r] + j) under the stride
 * conventions, bytes, offsets, statuses and guarantees of the uniform device forms -- offsets and status always written, nothing
 * written when the files do not fit cap, no read outside a file's own range, the outputs of an image with a nonzero status zeroed
 * (headers [n][9], K [n][T], idx [n][T][max_K]).  A file whose R or any block count differs from the call's -- also one with the
 * call's T split differently, written as (4, 1) and read as (1, 4) -- has IREC_REC_E_STRUCTURE.  blocks_per_res is a HOST array of
 * n_res_blocks <= IREC_REC_RAGGED_MAX_RES entries: its prefix sums travel by value in the kernel arguments, so these entry points too
 * allocate nothing and copy nothing.  More residual blocks than that, an entry < 1 or a T above INT32_MAX: IREC_E_INVALID with the
 * cause in irec_last_error, nothing launched, the outputs untouched.  The workspace is irec_rec_device_workspace_bytes's. */
#define IREC_REC_RAGGED_MAX_RES 64
irec_status irec_rec_encode_files_device_ragged(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                uint32_t channels, int32_t n_images, int32_t n_res_blocks,
                                                const int32_t *blocks_per_res /*host [n_res_blocks]*/, int32_t max_K,
                                                const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                uint8_t *out, int64_t cap, int64_t *offsets /*[n_images + 1]*/, int32_t *status /*[n_images]*/,
                                                void *workspace, size_t workspace_bytes, void *hip_stream);
irec_status irec_rec_decode_files_device_ragged(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                const int32_t *blocks_per_res /*host [n_res_blocks]*/, int32_t max_K,
                                                uint32_t *headers /*[n][9]*/, int32_t *K, int32_t *idx, int32_t *status, void *workspace,
                                                size_t workspace_bytes, void *hip_stream);

/* Empirical symbol tables (the reference's index_counts_file / num_aux_var_counts_file, rec/io/utils.py:31-56, 173-190) on the batched
 * and the device paths.  A table of n symbols is its cumulative counts cum [n + 1]: cum[0] = 0, cum[n] <= 2^30, symbol m over
 * [cum[m], cum[m + 1]); symbol 0 is the terminator and symbol m >= 1 the value m - 1, so a table codes the values [0, n - 2].
 * irec_rec_tables_build: cum from counts [n_symbols]; n_symbols >= 2, every count >= 1 and their sum <= 2^30, else IREC_E_INVALID
 *   with the cause in irec_last_error and cum untouched.
 * index_cum [n_index_symbols + 1]: the one table of every index stream.  count_cum [n_count_cum] with count_first [n_res_blocks + 1]:
 *   one table per residual block, back to back, that of residual block r at count_cum[count_first[r] .. count_first[r + 1]).
 *   Either of index_cum and count_cum may be NULL: the default model for that kind of stream.
 * Writing: a kind coded under a table sets its header word (6: counts, 7: indices); with count tables the largest-K words are
 *   0xFFFFFFFF.  A value without a symbol in its table is IREC_REC_E_INDEX_RANGE / IREC_REC_E_K_RANGE; the header keeps max_index.
 *   Without tables the bytes are those of the entry points above.
 * Reading: the FILE's two header words decide, per kind -- set and the call has that table: the table; set and no table:
 *   IREC_REC_E_COUNT_FILES; clear: the default model, whatever the call brought.  One call reads files of both sorts.  With the count
 *   word set the bound on K is the table's (n_r - 2) and the call's max_K.
 * A table is caller data: an entry under which the coder could not terminate (cum[0] != 0, cum[n] > 2^30, cum[m] >= cum[m + 1]) or a
 *   count_first that leaves count_cum gives that image IREC_REC_E_TABLE; no loop runs on and no read leaves the arrays as described.
 * The host forms take the ragged layout (blocks_per_res [R]; a uniform one is R equal entries), run on n_threads threads and report
 *   per image: offsets [n_images + 1] and status [n_images] always written, a file with a nonzero status has no bytes; the writer
 *   returns the total (also when > cap: nothing written, call again), -1 for bad arguments; the reader zeroes the outputs of an image
 *   with a nonzero status.  The device forms keep the stride conventions, guarantees and workspace of
 *   irec_rec_encode_files_device_ragged / irec_rec_decode_files_device_ragged; the tables are DEVICE pointers, blocks_per_res a host
 *   array: no allocation, no synchronisation, no copy to the host.  An index table of at most IREC_REC_TABLE_LDS_SYMBOLS symbols is
 *   staged in LDS by every workgroup that codes index streams (16 KB + 4 B at the limit: a 256-lane workgroup of these latency-bound
 *   lanes then still shares a CU's 160 KB with eight others, and the limit covers every sample count the coders here draw, S <= 4096
 *   being rows of at most 4095 values plus the terminator); a larger one is read from global memory. */
#define IREC_REC_TABLE_LDS_SYMBOLS 4096
irec_status irec_rec_tables_build(const int64_t *counts, int32_t n_symbols, uint32_t *cum /*[n_symbols + 1]*/);
int64_t irec_rec_encode_files_tables(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                     uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                     int32_t max_K, const int32_t *K /*[n][T]*/, const int32_t *idx /*[n][T][max_K]*/,
                                     const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum,
                                     const int32_t *count_first /*[R + 1]*/, int64_t n_count_cum, uint8_t *out, int64_t cap,
                                     int64_t *offsets /*[n_images + 1]*/, int32_t *status /*[n_images]*/, int32_t n_threads);
irec_status irec_rec_decode_files_tables(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                         const int32_t *blocks_per_res, int32_t max_K, const uint32_t *index_cum, int32_t n_index_symbols,
                                         const uint32_t *count_cum, const int32_t *count_first, int64_t n_count_cum,
                                         uint32_t *headers /*[n][9]*/, int32_t *K /*[n][T]*/, int32_t *idx /*[n][T][max_K]*/,
                                         int32_t *status /*[n]*/, int32_t n_threads);
irec_status irec_rec_encode_files_device_tables(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                uint32_t channels, int32_t n_images, int32_t n_res_blocks,
                                                const int32_t *blocks_per_res /*host [n_res_blocks]*/, int32_t max_K,
                                                const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum,
                                                const int32_t *count_first, int64_t n_count_cum, uint8_t *out, int64_t cap,
                                                int64_t *offsets /*[n_images + 1]*/, int32_t *status /*[n_images]*/, void *workspace,
                                                size_t workspace_bytes, void *hip_stream);
irec_status irec_rec_decode_files_device_tables(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                const int32_t *blocks_per_res /*host [n_res_blocks]*/, int32_t max_K,
                                                const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum,
                                                const int32_t *count_first, int64_t n_count_cum, uint32_t *headers /*[n][9]*/, int32_t *K,
                                                int32_t *idx, int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream);
/* Segmented files (NAME.recs): an opt-in second container for few, long streams.  The rows of every residual block
 * are cut into segments of segment_blocks coder blocks (the last one of a residual block may be shorter); every segment is a pair of
 * ordinary streams -- exactly what the plain container holds for those blocks alone, the count model's nav_max the segment's largest
 * K -- and one lane, or one host thread's turn, codes one stream of one segment.  Default symbol models only.
 *   0 "IRSG" | 4 version u16 = 1, reserved u16 = 0 | 8 the 28-byte static header of .rec, both flags 0 | 36 segment_blocks u32 |
 *   40 R x u32 blocks | directory: for r, for s < ceil(blocks[r] / segment_blocks): max_part, count_bytes, index_bytes as u32 |
 *   the streams in directory order, a segment's count stream before its index stream.
 * All four take the ragged layout (blocks_per_res, a HOST array of n_res_blocks <= IREC_REC_RAGGED_MAX_RES entries; the uniform case
 * is a constant array) and rows K [n][T], idx [n][T][max_K]; at most 2^22 segments per image.  They report per image: offsets
 * [n_images + 1] and status [n_images] always written, a file with a nonzero status has no bytes, nothing at all is written when the
 * files do not fit cap (offsets still say what they take); the reader zeroes headers, K and idx of an image with a nonzero status.
 * The reader holds magic, version, flags, R, the block counts and segment_blocks against the call, wants header + directory + the
 * listed streams to be the file's length exactly and every max_part <= max_K, and never reads outside a file's own range.
 * The host forms run on n_threads threads over (image, segment) and give byte for byte what the device forms give; the writer
 * returns the total, -1 for bad arguments.  The device forms follow irec_rec_encode_files_device_ragged: device pointers under the
 * same stride conventions, asynchronous on hip_stream, no allocation, no copy; workspace of irec_rec_seg_workspace_bytes (0 for
 * arguments the calls would refuse), 8-byte aligned.  The plain readers refuse such a file (its bytes 26..27, their R, are the high
 * half of a width below 65536: no residual blocks). */
size_t irec_rec_seg_workspace_bytes(int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res, int32_t segment_blocks);
int64_t irec_rec_encode_files_segmented(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                        uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                        int32_t segment_blocks, int32_t max_K, const int32_t *K /*[n][T]*/,
                                        const int32_t *idx /*[n][T][max_K]*/, uint8_t *out, int64_t cap,
                                        int64_t *offsets /*[n_images + 1]*/, int32_t *status /*[n_images]*/, int32_t n_threads);
irec_status irec_rec_decode_files_segmented(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                            const int32_t *blocks_per_res, int32_t segment_blocks, int32_t max_K,
                                            uint32_t *headers /*[n][9]*/, int32_t *K /*[n][T]*/, int32_t *idx /*[n][T][max_K]*/,
                                            int32_t *status /*[n]*/, int32_t n_threads);
irec_status irec_rec_encode_files_device_segmented(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                   uint32_t channels, int32_t n_images, int32_t n_res_blocks,
                                                   const int32_t *blocks_per_res /*host [n_res_blocks]*/, int32_t segment_blocks,
                                                   int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx,
                                                   int64_t idx_stride, uint8_t *out, int64_t cap, int64_t *offsets /*[n_images + 1]*/,
                                                   int32_t *status /*[n_images]*/, void *workspace, size_t workspace_bytes,
                                                   void *hip_stream);
irec_status irec_rec_decode_files_device_segmented(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                   const int32_t *blocks_per_res /*host [n_res_blocks]*/, int32_t segment_blocks,
                                                   int32_t max_K, uint32_t *headers /*[n][9]*/, int32_t *K, int32_t *idx, int32_t *status,
                                                   void *workspace, size_t workspace_bytes, void *hip_stream);

/* Histograms of packed rows, to fit tables from: K [n_images][T] and idx [n_images][T][max_K] under the stride conventions above, added
 * INTO uint64 arrays (a corpus is fed batch by batch; zero them first):
 *   index_hist [n_index_values]                  the first K indices of every row whose K lies in [0, min(max_K, n_count_values - 1)];
 *   count_hist [n_res_blocks][n_count_values]    the K of every row, by its residual block;
 *   streams [1 + n_res_blocks]                   streams seen: [0] index streams (n_images R), [1 + r] count streams of block r (n_images);
 *   rejected [1]                                 values outside their range (a K outside [0, n_count_values) or above max_K -- its row's
 *                                                indices are then not looked at --, an index outside [0, n_index_values)): not counted.
 * Integer adds only: the result does not depend on the order of the adds.  The device form (csrc/irec_rec_tables.hip) keeps the bins
 * of a workgroup in LDS and adds every non-empty one to global memory once; asynchronous on hip_stream, nothing allocated or copied. */
irec_status irec_rec_hist_rows(int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res, int32_t max_K, const int32_t *K,
                               int64_t k_stride, const int32_t *idx, int64_t idx_stride, int32_t n_index_values, int32_t n_count_values,
                               uint64_t *index_hist, uint64_t *count_hist, uint64_t *streams, uint64_t *rejected);
irec_status irec_rec_hist_rows_device(int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res /*host*/, int32_t max_K,
                                      const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride, int32_t n_index_values,
                                      int32_t n_count_values, uint64_t *index_hist, uint64_t *count_hist, uint64_t *streams,
                                      uint64_t *rejected, void *hip_stream);

/* The verdict on the rows a decode call is about to read, on the device (csrc/irec_rows.hip over csrc/irec_rows_core.h).  The decode
 * entry points above answer a row they cannot decode with p_loc, silently; a caller whose rows never leave the device (the output of
 * irec_rec_decode_files_device) gets the cause here, per image, without a copy to the host.
 * A group is one image's blocks in one residual block: blocks j < blocks_per_group, block j at row b = block_row[g * blocks_per_group + j]
 * (device int32; NULL: g * blocks_per_group + j), its count at K[b * k_stride], its indices at idx[b * idx_stride + t] -- the stride
 * conventions of irec_rec_encode_files_device: the packed arrays or one joined [rows][1 + width] tensor pass unchanged.
 * status[g] becomes the first cause of the group's LOWEST failing block:
 *   K < min_K or K > max_K: IREC_ROWS_E_K_RANGE (min_K: 0 for the beam-search coder, 1 for the sequential one);
 *   K > k_limit: IREC_ROWS_E_RATIO_TABLE (k_limit: the length of the fitted ratio table, INT32_MAX with extrapolated ratios);
 *   an index outside [0, n_samples) among the first K: IREC_ROWS_E_INDEX_RANGE.
 * A nonzero status[g] already present is kept: the launches of successive residual blocks on one stream accumulate the first cause per
 * image (one workgroup per group, one lane reads and writes status[g]; no atomics).  No read goes past idx[b * idx_stride + max_K - 1],
 * whatever K holds.  Asynchronous on hip_stream: no allocation, no synchronisation. */
typedef enum { IREC_ROWS_OK = 0, IREC_ROWS_E_K_RANGE = 1, IREC_ROWS_E_INDEX_RANGE = 2, IREC_ROWS_E_RATIO_TABLE = 3 } irec_rows_status;
irec_status irec_decode_rows_status(int64_t n_groups, int32_t blocks_per_group, const int32_t *block_row /* NULL: g * bpg + j */,
                                    const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride, int32_t max_K,
                                    int32_t min_K, int32_t k_limit, int32_t n_samples, int32_t *status /* [n_groups] */,
                                    void *hip_stream);

/* The .res container (csrc/irec_res.hip over csrc/irec_res_core.h): the pixels of an image, arithmetic-coded under the model's
 * discretized-logistic likelihood given its reconstruction, so that .rec + .res decode to exactly the uint8 image.  .rec files are
 * untouched by it.  pixels [n][channels][height][width] uint8, loc the same shape in float32 (the clamped reconstruction), scale the
 * call's one likelihood scale in [2^-24, 2^24].  A pixel's model is a function of the integer rint(loc * 4096) and of scale alone
 * (INTEGRATION.md has the counts and the file layout).  An image is channels * height * width symbols cut into streams of stream_len
 * (1 .. 4096), n_streams = ceil(symbols / stream_len), one lane per stream.
 * The device entry points follow irec_rec_encode_files_device: device pointers, asynchronous on hip_stream, no allocation,
 * synchronisation or copy inside; offsets [n_images + 1] and status [n_images] are always written; nothing is written into out when
 * offsets[n_images] > cap; a file with a nonzero status has no bytes; the reader leaves no file's [offsets[i], offsets[i + 1]) and an
 * image with a nonzero status has its pixels zeroed.  The host forms run the same core over host memory on n_threads threads
 * (0 = one per core, at most 32) and give the same bytes, pixels and statuses.
 * irec_res_model_counts: the 257 cumulative counts C(0 .. 256) of one (m, scale); irec_res_symbol_counts: count[e] = C(x + 1) - C(x) of
 * every pixel (its ideal length is -log2(count / 65536)), 0 where loc is not finite. */
typedef enum {
  IREC_RES_OK = 0,
  IREC_RES_E_SCALE = 1,             /* encode: the scale is not finite, not positive or outside [2^-24, 2^24]              */
  IREC_RES_E_LOC = 2,               /* encode: a loc that is not finite                                                   */
  IREC_RES_E_TRUNCATED_HEADER = 3,  /* decode: fewer bytes than the header and its stream lengths                         */
  IREC_RES_E_MAGIC = 4,             /* decode: not the magic word or not this version                                     */
  IREC_RES_E_SHAPE = 5,             /* decode: height, width, channels or stream_len differ from the call's               */
  IREC_RES_E_SCALE_WORD = 6,        /* decode: the file's scale word differs from the call's                              */
  IREC_RES_E_TRUNCATED_STREAMS = 7, /* decode: the streams run past the file                                              */
  IREC_RES_E_CORRUPT = 8,           /* decode: a stream with target < 0, width <= 0 or its shift budget spent             */
  IREC_RES_E_CHECKSUM = 9           /* decode: the pixels do not sum to the header's checksum (another loc, damaged bits) */
} irec_res_status;
size_t irec_res_device_workspace_bytes(int32_t n_images, int64_t n_streams);
irec_status irec_res_encode_files_device(const uint8_t *pixels, const float *loc, float scale, int32_t n_images, uint32_t height,
                                         uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap,
                                         int64_t *offsets /*[n_images + 1]*/, int32_t *status /*[n_images]*/, void *workspace,
                                         size_t workspace_bytes, void *hip_stream);
irec_status irec_res_decode_files_device(const uint8_t *bytes, const int64_t *offsets, const float *loc, float scale, int32_t n_images,
                                         uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *pixels_out,
                                         int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream);
irec_status irec_res_encode_files(const uint8_t *pixels, const float *loc, float scale, int32_t n_images, uint32_t height, uint32_t width,
                                  uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status,
                                  int32_t n_threads);
irec_status irec_res_decode_files(const uint8_t *bytes, const int64_t *offsets, const float *loc, float scale, int32_t n_images,
                                  uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *pixels_out,
                                  int32_t *status, int32_t n_threads);
irec_status irec_res_model_counts(int32_t m, float scale, uint32_t *cumulative /*[257]*/);
irec_status irec_res_symbol_counts(const uint8_t *pixels, const float *loc, float scale, int64_t n, uint32_t *count /*[n]*/);

/* One scale per channel: .res version 2.  The four "_scales" entry points take the arguments of the four above with
 * scales [channels] (float32; a device pointer in the device forms) in place of scale, and keep their guarantees and their
 * workspace (irec_res_device_workspace_bytes).  Symbol p of an image belongs to channel p / (height * width); a stream that crosses a
 * channel boundary goes on under the next channel's scale; the model of a pixel given (m, s_c) is the same.  The file differs from
 * version 1 in the version word (2) and in holding channels scale words where version 1 holds one (INTEGRATION.md has the offsets).
 * Any channel's scale outside [2^-24, 2^24] or not finite: IREC_RES_E_SCALE for every image.  Any scale word that differs from the
 * call's: IREC_RES_E_SCALE_WORD.  A version-1 file given to a "_scales" reader, or a version-2 file given to a reader above:
 * IREC_RES_E_MAGIC. */
irec_status irec_res_encode_files_device_scales(const uint8_t *pixels, const float *loc, const float *scales /*[channels]*/, int32_t n_images,
                                                uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *out,
                                                int64_t cap, int64_t *offsets /*[n_images + 1]*/, int32_t *status /*[n_images]*/,
                                                void *workspace, size_t workspace_bytes, void *hip_stream);
irec_status irec_res_decode_files_device_scales(const uint8_t *bytes, const int64_t *offsets, const float *loc, const float *scales /*[channels]*/,
                                                int32_t n_images, uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len,
                                                uint8_t *pixels_out, int32_t *status, void *workspace, size_t workspace_bytes,
                                                void *hip_stream);
irec_status irec_res_encode_files_scales(const uint8_t *pixels, const float *loc, const float *scales /*[channels]*/, int32_t n_images,
                                         uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap,
                                         int64_t *offsets, int32_t *status, int32_t n_threads);
irec_status irec_res_decode_files_scales(const uint8_t *bytes, const int64_t *offsets, const float *loc, const float *scales /*[channels]*/,
                                         int32_t n_images, uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len,
                                         uint8_t *pixels_out, int32_t *status, int32_t n_threads);

/* What a batch costs under candidate scales (csrc/irec_res_fit.hip over csrc/irec_res_fit_core.h): the quantity a fitter of the .res
 * scale searches over.  pixels, loc [n][channels][height][width] as above; scales [channels][n_candidates] float32,
 * 1 <= n_candidates <= IREC_RES_FIT_MAX_CANDIDATES; cost [IREC_RES_COST_ENTRIES] from irec_res_cost_table:
 * cost[n] = rint((16 - log2 n) * 2^16) for n in 1 .. 65536, cost[0] = 0 (data: built once on the host, passed to both forms).
 *   bits [n][channels][n_candidates] int64, written (not added): the sum over the pixels of image i, channel ch of
 *        cost[C(x + 1) - C(x)] under scales[ch][k] -- the model's exact code length in units of 2^-16 bit; INT64_MAX for a candidate
 *        outside [2^-24, 2^24] or not finite (no error)
 *   skipped [n][channels] int64: the pixels left out of every sum because their loc is not finite
 * Integer adds only: the result depends on no order, the device form equals the host form bit for bit, and an image's rows are the
 * same alone or inside any batch.  The device form: device pointers (cost and scales too), asynchronous on hip_stream, no allocation,
 * synchronisation, copy or atomic inside (two launches); it writes exactly bits, skipped and the workspace (8-byte aligned, at least
 * irec_res_scale_bits_workspace_bytes, which is 0 for a shape the entries refuse).  Null pointers, a shape the .res entries refuse,
 * n_candidates outside 1 .. 64: IREC_E_INVALID; a workspace smaller than sized: IREC_E_WORKSPACE; no launch either way. */
#define IREC_RES_FIT_MAX_CANDIDATES 64
#define IREC_RES_COST_ENTRIES 65537
irec_status irec_res_cost_table(uint32_t *cost /*[IREC_RES_COST_ENTRIES]*/);
size_t irec_res_scale_bits_workspace_bytes(int32_t n_images, uint32_t height, uint32_t width, uint32_t channels, int32_t n_candidates);
irec_status irec_res_scale_bits_device(const uint8_t *pixels, const float *loc, const float *scales, const uint32_t *cost, int32_t n_images,
                                       uint32_t height, uint32_t width, uint32_t channels, int32_t n_candidates, int64_t *bits,
                                       int64_t *skipped, void *workspace, size_t workspace_bytes, void *hip_stream);
irec_status irec_res_scale_bits(const uint8_t *pixels, const float *loc, const float *scales, const uint32_t *cost, int32_t n_images,
                                uint32_t height, uint32_t width, uint32_t channels, int32_t n_candidates, int64_t *bits, int64_t *skipped,
                                int32_t n_threads);

/* Distortion of a batch (csrc/irec_quality.hip over csrc/irec_quality_core.h): what PSNR and MS-SSIM are made from, for a
 * (reconstruction) and b (original), float32 [n][c][h][w] each.  A pixel is v * mul + add, clamped to [0, max_val] where the image's
 * clip flag is set; MS-SSIM is tf.image.ssim_multiscale of TF 2.1 with filter_size 11 and filter_sigma 1.5 (INTEGRATION.md has the
 * definition), n_scales 1 .. 5 scales, every scale at least 11 x 11.  Outputs:
 *   per_scale [n][c][n_scales][2]  the means over the VALID filter outputs of lum * cs and of cs, NOT clamped at 0
 *   sse [n]                        the sum over the image's c * h * w pixels of (pixel_a - pixel_b)^2
 * The caller finishes: psnr = 20 log10(max_val) - 10 log10(sse / (c h w)); ms_ssim = mean over channels of
 * prod_{k < last} max(cs_k, 0)^pf_k * max(ssim_last, 0)^pf_last.
 * The device entry follows irec_res_encode_files_device: device pointers, asynchronous on hip_stream, no allocation, synchronisation
 * or copy inside (n_scales + 1 launches); it writes exactly per_scale and sse, and the workspace (256-byte aligned, at least
 * irec_quality_workspace_bytes, which is 0 for a shape the entries refuse).  A result is the same bits from run to run and for an
 * image alone or inside any batch; an image with a NaN pixel has non-finite results and changes no other image's.
 * irec_quality_host runs the same core over host memory on n_threads threads (0 = one per core, at most 32): the same outputs
 * whatever n_threads is.  Null pointers, n_scales outside 1 .. 5, an image below 11 x 11 at one of its scales, a max_val that is
 * not positive: IREC_E_INVALID; a workspace smaller than sized: IREC_E_WORKSPACE; no launch either way. */
typedef struct {
  float mul_a, add_a, mul_b, add_b; /* pixel = v * mul + add                                   */
  int32_t clip_a, clip_b;           /* nonzero: the pixel is clamped to [0, max_val]           */
  float max_val, k1, k2;            /* c1 = (k1 max_val)^2, c2 = (k2 max_val)^2; TF: .01, .03  */
} irec_quality_params;
size_t irec_quality_workspace_bytes(int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_scales);
irec_status irec_quality_device(const float *a, const float *b, int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_scales,
                                const irec_quality_params *params, float *per_scale, float *sse, void *workspace,
                                size_t workspace_bytes, void *hip_stream);
irec_status irec_quality_host(const float *a, const float *b, int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_scales,
                              const irec_quality_params *params, float *per_scale, float *sse, int32_t n_threads);

/* ---- the ideal half of a results row: seeded posterior draws with their KL, and the log-likelihood of a batch ----------------------
 * (csrc/irec_ideal.hip over csrc/irec_ideal_core.h, which writes every operation sequence down.)  What the reference's evaluation
 * drivers take from a sampling forward pass `model(image)`: the latents are draws from the posteriors, KL is the closed form, and the
 * residual is minus the discretized-logistic log-likelihood of the image under the clipped reconstruction.
 *
 * irec_posterior_draw_*: n_images images of `dims` contiguous float32 each; mq, sq, mp, sp are four separate arrays
 * [n_images][dims] (posterior loc and scale, prior loc and scale).  Outputs:
 *   sample [n_images][dims] float32   mq + sq * eps(seed, tag, image_base + i, e): one rounding for the product, one for the sum
 *   kl [n_images] float64             sum over e of KL(N(mq, sq) || N(mp, sp)) in nats, every term in float64
 * The noise is this library's OWN seeded stream, not TensorFlow's (the reference's pass is unseeded: there is nothing to be faithful
 * to): Philox4x32-10 under the key (seed lo32, seed hi32) of the int64 seed in two's complement -- any int64 is a valid seed -- and the
 * counter (block lo32, block hi32, image number, tag); element e takes word e & 3 of block e >> 2; u = ((word >> 8) + 0.5) 2^-24;
 * eps = (float)ndtri64(u), the Cephes rational form in float64 over the library's deterministic log and IEEE sqrt, so |eps| < 5.5.
 * tag names the tensor (a residual block's index, a level).  image_base + i lies in [0, 2^32).  A draw is a property of
 * (seed, tag, image number, e) only: image i of a batch with base b has the bits of a one-image call with base b + i.
 *
 * irec_loglik_*: x (the image) and loc (the clipped reconstruction), float32 [n_images][channels][plane] each, plane = h w;
 * log_scales float32 [n_scales], n_scales 1 (one scale) or channels; scale = exp(log_scale).  Output ll [n_images] float64, nats:
 *   a = (floor(x / binsize) binsize - loc) / scale;  ll = sum of log(sigmoid(a + binsize / scale) - sigmoid(a) + 1e-7)
 * in float64 after widening the float32 inputs (rec/models/resnet_vae.py:640-650).
 *
 * The device entries follow irec_quality_device: device pointers (log_scales too), asynchronous on hip_stream, no allocation,
 * synchronisation, copy or atomic inside (two launches each), capturable into a HIP graph; they write exactly their outputs and
 * the workspace (8-byte aligned, at least irec_ideal_workspace_bytes(n_images, dims) bytes, dims = channels plane for the
 * likelihood; 0 for a shape the entries refuse).  A sum is added in a fixed order -- lanes of a tile of IREC_IDEAL_TILE elements, tiles
 * of an image -- so a result is the same bits from run to run and for an image alone or inside any batch, and a NaN in one image
 * reaches that image's outputs only.  The host entries run the same core over host memory on n_threads threads (0 = one per core, at
 * most 32) and give the device's bits, whatever n_threads is.  Null or misaligned pointers (float32 arrays 4 bytes, float64 8),
 * n_images < 1, dims outside 1 .. 2^40, an image number outside [0, 2^32), n_scales neither 1 nor channels, a binsize that is not
 * positive and finite: IREC_E_INVALID; a workspace smaller than sized: IREC_E_WORKSPACE; no launch either way. */
#define IREC_IDEAL_TILE 4096
size_t irec_ideal_workspace_bytes(int32_t n_images, int64_t dims);
irec_status irec_posterior_draw_device(const float *mq, const float *sq, const float *mp, const float *sp, int32_t n_images, int64_t dims,
                                       int64_t seed, uint32_t tag, int64_t image_base, float *sample, double *kl, void *workspace,
                                       size_t workspace_bytes, void *hip_stream);
irec_status irec_posterior_draw_host(const float *mq, const float *sq, const float *mp, const float *sp, int32_t n_images, int64_t dims,
                                     int64_t seed, uint32_t tag, int64_t image_base, float *sample, double *kl, int32_t n_threads);
irec_status irec_loglik_device(const float *x, const float *loc, const float *log_scales, int32_t n_scales, int32_t n_images,
                               int32_t channels, int64_t plane, double binsize, double *ll, void *workspace, size_t workspace_bytes,
                               void *hip_stream);
irec_status irec_loglik_host(const float *x, const float *loc, const float *log_scales, int32_t n_scales, int32_t n_images, int32_t channels,
                             int64_t plane, double binsize, double *ll, int32_t n_threads);

/* ---- the driver's resize: a batch of images shrunk bilinearly (csrc/irec_image.hip over csrc/irec_image_core.h) --------------------
 * Replaces `tf.image.resize(image, [h - h % 64, w - w % 64])` of examples/lossy/compress_with_lossy_model.py:183-184: TF 2.1
 * ResizeBilinear with half_pixel_centers=True and antialias=False, float32 throughout, IEEE operations only (DESIGN.md §3 "resize"
 * and the core header write the operation sequence down).  src: n images of c channels, in_h x in_w, as [n][c][in_h][in_w]
 * (IREC_IMAGE_NCHW) or [n][in_h][in_w][c] (IREC_IMAGE_NHWC), float32 (IREC_IMAGE_F32) or uint8 (IREC_IMAGE_U8: v = u / 255 on load);
 * dst: the same layout with out_h x out_w, float32.  SHRINK ONLY: out_h <= in_h and out_w <= in_w (the driver never enlarges); an
 * axis of equal sizes is not interpolated, so equal sizes are a bit-for-bit copy (of u / 255 for a uint8 source).
 * The device entry follows irec_quality_device: device pointers, asynchronous on hip_stream, one launch, no workspace, allocation,
 * synchronisation, copy or atomic inside, capturable into a HIP graph; it writes exactly dst.  A result is a function of the image
 * and the sizes only: the same bits from run to run and for an image alone or inside any batch; a NaN or an infinity reaches the
 * outputs that have it among their four taps and no other.  irec_resize_bilinear_host runs the same core over host memory on
 * n_threads threads (0 = one per core, at most 32) and gives the device's bits, whatever n_threads is.  Null or misaligned pointers,
 * a count or size below 1, out > in on either axis, a side above 65536, an unknown layout or dtype: IREC_E_INVALID, no launch, dst
 * untouched. */
#define IREC_IMAGE_NCHW 0
#define IREC_IMAGE_NHWC 1
#define IREC_IMAGE_F32 0
#define IREC_IMAGE_U8 1
irec_status irec_resize_bilinear_device(const void *src, int32_t src_dtype, int32_t n, int32_t c, int32_t in_h, int32_t in_w, int32_t out_h,
                                        int32_t out_w, int32_t layout, float *dst, void *hip_stream);
irec_status irec_resize_bilinear_host(const void *src, int32_t src_dtype, int32_t n, int32_t c, int32_t in_h, int32_t in_w, int32_t out_h,
                                      int32_t out_w, int32_t layout, float *dst, int32_t n_threads);

#ifdef __cplusplus
}
#endif
#endif /* IREC_H_ */
