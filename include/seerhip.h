/*
 * seerhip.h -- flat C ABI of libseerhip.so, the MI355X (gfx950) per-variant association engine.
 *
 * The reference (pyseer) is pure Python and has NO FFI for this path; the boundary it exposes is the
 * Python call signature between its variant stream and its per-variant test:
 *     pyseer/model.py:202  fixed_effects_regression(variant,p,k,m,c,af,pattern,lineage_effects,lin,pret,lrtt,
 *                                                   null_res,null_firth,kstrains,nkstrains,continuous) -> Seer
 *     pyseer/lmm.py:125    fit_lmm(lmm,h2,variants,variant_mat,lineage_effects,lineage_clusters,covariates,
 *                                  continuous,filter_pvalue,lrt_pvalue) -> [LMM]
 *     pyseer/lmm.py:228    fit_lmm_block(lmm,h2,variant_block) -> {beta,bse,frac_h2,p_values}
 * Each entry point below names the reference call it replaces.  INTEGRATION.md shows the ctypes stub a
 * pyseer maintainer would add (pyseer_amd/_abi.py is that stub, in full).
 *
 * Conventions
 *  - return 0 on success, a negative SH_E* code otherwise; sh_last_error() gives a thread-local message.
 *  - no CPU fallback: every compute entry point needs a gfx950 device (sh_create fails without one).
 *  - host-pointer calls (sh_*_batch) copy in/out and synchronise; *_dev calls take DEVICE pointers, are
 *    asynchronous on the context's stream (sh_set_stream) and touch no host memory.
 *  - a context is bound to one device and is NOT thread-safe; use one context per device per host thread.
 *  - presence bits: V rows x row_bytes bytes, variant-major; bit (i & 7) of byte (i >> 3) of row v is the
 *    presence of sample i in variant v (LSB first).  Bits at i >= n_samples are ignored.
 *  - flags[v]: bits 0..8 = notes in the order of docs/usage.rst:553-566 (SH_NOTE_*), bit 18 = SH_FLAG_FIRTH_SENSITIVE, bit 16 = Seer/LMM.prefilter,
 *    bit 17 = Seer/LMM.filter.
 */
#ifndef SEERHIP_H
#define SEERHIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SH_ABI_VERSION 2

#define SH_OK          0
#define SH_EINVAL     -1   /* bad argument / call order */
#define SH_ENODEV     -2   /* no gfx950 device / device error */
#define SH_ENOMEM     -3
#define SH_EH2        -4   /* h2 outside [0,1): reference raises KeyError('beta') (lmm_cov.py:667-670) */
#define SH_ESHAPE     -5   /* shape mismatch: reference AssertionError (lmm_cov.py:674) */
#define SH_EHIP       -6   /* HIP runtime failure */

/* notes (pyseer/model.py:253-386, pyseer/lmm.py:160-204) */
#define SH_NOTE_AF_FILTER        (1u << 0)
#define SH_NOTE_PRE_FILTER       (1u << 1)
#define SH_NOTE_BAD_CHISQ        (1u << 2)
#define SH_NOTE_HIGH_BSE         (1u << 3)
#define SH_NOTE_PERFECT_SEP      (1u << 4)
#define SH_NOTE_MATRIX_INV       (1u << 5)
#define SH_NOTE_FIRTH_FAIL       (1u << 6)
#define SH_NOTE_MISSING_DATA     (1u << 7)
#define SH_NOTE_LRT_FILTER       (1u << 8)
#define SH_FLAG_PREFILTER        (1u << 16)
#define SH_FLAG_FILTER           (1u << 17)
/* A row fitted by fit_firth (model.py:414-504) on which the REFERENCE's own answer is fragile -- it may depend on the order of the reference's
 * floating-point sums.  Set when
 *   (a) the variant all but separates the phenotype: a cell of its 2 x 2 table holds at most one sample.  Every `firth-fail` the reference
 *       itself was seen to return (tests/golden/glm_exit_firthfail_*.npz: 13 rows, N = 300 ... 5000) is such a row: near its stop
 *       `firth_likelihood(new) > firth_likelihood(old)` (model.py:467) compares values one ulp apart, for 1000 halvings if the last bits
 *       fall that way, and the reference fits the same row with the samples in another order.  Nothing order-independent tells those rows
 *       from their neighbours that the reference fits (profiles/r05/firthfail_trace.txt), so the whole class is marked;
 *   (b) the iteration took 12 or more accepted steps (linear convergence), or its stop rule (model.py:477-479) was met within 1e-8 of the
 *       limit: the answer then moves by a whole step (~1e-4) with the last bit of a norm;
 *   (c) this library itself reports firth-fail (SEERHIP_ROUTE firth_literal / firth_strict).
 * Informational: set beside the row's statistics, never a reason to filter; < 1e-3 of the rows of a forced-Firth run on random k-mers.
 * DESIGN.md section 6. */
#define SH_FLAG_FIRTH_SENSITIVE  (1u << 18)

typedef struct sh_ctx sh_ctx;

int         sh_abi_version(void);
const char *sh_last_error(void);
int         sh_device_count(void);
/* Start the HIP runtime on `device` and load this library's code object (a no-op launch): about 0.8 s of driver work on first use, which
 * a caller can run on a side thread while it reads its inputs (the reference has no counterpart: its workers start with the interpreter).
 * Optional: every other entry point initialises what it needs. */
int         sh_warmup(int device);

/* How host threads wait for the device: sleeping != 0 asks for waits that SLEEP (hipDeviceScheduleBlockingSync, offered to each device at its
 * first sh_warmup / sh_create; a device that something else initialised first keeps its mode).  The runtime's default is to spin: one CPU per
 * waiting stream -- fine for a benchmark, not for a job of several device streams under a CPU quota (the command line asks for sleeping
 * waits).  Call before the first sh_warmup / sh_create.  Process-wide. */
void        sh_set_wait_mode(int sleeping);

/* one context per device; n_samples = len(p) of the reference (at least 1: a context of a single sample serves the readers that tokenise on
 * the device -- no model can be set up on it, as none can be fitted to one sample) */
sh_ctx *sh_create(int device, int n_samples);
void    sh_destroy(sh_ctx *ctx);
/* enqueue all later work on this hipStream_t (NULL = the device's default stream) */
int     sh_set_stream(sh_ctx *ctx, void *hip_stream);
int     sh_synchronize(sh_ctx *ctx);
/* HIP-event timing of the dominant kernel(s) of each later *_batch_dev call, recorded on the context's stream: the contraction kernel
 * (k_lmm_quadform_i8w, or k_lmm_quadform_i8 where the former's conditions do not hold; main pass) for the LMM; every fit kernel of a fixed-effects batch (Newton, Firth rounds, final pass; the bit repack is outside).
 * sh_get_timing synchronises on the recorded events and returns their sum. */
int     sh_set_timing(sh_ctx *ctx, int on);
int     sh_get_timing(sh_ctx *ctx, double *total_ms, int64_t *launches);
/* Pattern de-duplication (pyseer/input.py:710 hash_pattern, scripts/count_patterns.py): when on, every later
 * *_batch / *_batch_dev call tests each DISTINCT packed row once (exact row comparison, the hash only finds candidates) and fans
 * the result out to all variants that share it.  Outputs are unchanged.  Costs one stream synchronisation per batch.
 * sh_dedup_info: the number of rows the last batch (its last chunk) actually tested.  That is the number of distinct rows unless two
 * different rows share all 64 bits of the hash: the hash then belongs to the one with the lowest index, and the other row -- and every
 * duplicate of it, each on its own -- is tested as well.  So the count is an upper bound of the number of distinct patterns, and equal to
 * it for all practical input (tests/test_dedup_collisions_gpu.py constructs the exception). */
int     sh_set_dedup(sh_ctx *ctx, int on);
int     sh_dedup_info(sh_ctx *ctx, int64_t *unique_last_batch);
/* AF filter of the variant stream (pyseer/input.py:608,693): keep min_af <= count/n <= max_af (inclusive);
 * others get SH_NOTE_AF_FILTER | SH_FLAG_PREFILTER and NaN statistics.  Default: disabled (0, 1). */
int     sh_set_af_filter(sh_ctx *ctx, double min_af, double max_af);

/* ---------------------------------------------------------------------------------------------
 * LMM  (replaces pyseer/lmm.py:125 fit_lmm + :228 fit_lmm_block over pyseer/fastlmm/lmm_cov.py:165,597,686)
 * U: n x k row-major (lmm.U; arr_0 of the --save-lmm cache), S: k (lmm.S), y: n (lmm.Y),
 * C: n x D row-major covariates with the intercept LAST (lmm.X, pyseer/lmm.py:95-99), h2 (lmm.py:115).
 * continuous selects the prefilter test (model.py:52-55 vs :57-68); pret/lrtt = filter_pvalue/lrt_pvalue
 * (compared with >=, lmm.py:174,201).  n_limbs = 3..7 int8 limbs of the fixed-point kernel matrix; 0 = automatic:
 * the smallest of 4 and 5 whose typical a-posteriori bound on x^T K^-1 x is at most a quarter of the tolerance of sh_set_lmm_tol (1e-8; a variant
 * whose own bound exceeds the tolerance is re-contracted with the extra limbs whichever count was chosen; sh_lmm_info / sh_lmm_bound report both).
 * With pret < 1 a pre-filtered variant is not fitted and carries NaN statistics (fit_lmm); with pret >= 1 every AF-passing variant
 * carries its statistics (fit_lmm_block) and masking by the prefilter flag is the caller's.
 * ------------------------------------------------------------------------------------------- */
int sh_lmm_setup(sh_ctx *ctx, const double *U, const double *S, int k, const double *y,
                 const double *C, int D, double h2, int continuous, double pret, double lrtt, int n_limbs);
/* Multi-GPU (the counterpart of the reference's --cpu N workers sharing one LMM object, pyseer/__main__.py:541-568):
 * copy the per-run LMM state of `src` (after sh_lmm_setup) device-to-device into `dst`, a context on another (or the same) device with
 * the same n_samples.  One set-up per run instead of one per GPU; the per-variant path has no inter-GPU traffic at all. */
int sh_lmm_share(sh_ctx *dst, sh_ctx *src);
/* per variant: prep, pvalue, beta, bse, frac_h2 (each V doubles) + flags.  Statistics are written for every
 * variant that passes the AF filter (the caller applies the NaN masking implied by flags, lmm.py:176-217). */
int sh_lmm_batch(sh_ctx *ctx, const uint8_t *bits, int64_t row_bytes, int64_t V,
                 double *prep, double *pvalue, double *beta, double *bse, double *frac_h2, uint32_t *flags);
/* Pipelined form of the host-pointer batches (the counterpart of the reference's pool.imap over blocks of variants, pyseer/__main__.py:541-568:
 * block k+1 is submitted while block k's results are still being produced).  sh_lmm_batch_async / sh_glm_batch_async take the arguments of
 * sh_lmm_batch / sh_glm_batch, stage all of `bits` (the caller may release it on return) and queue the batch, but return while its LAST
 * chunk is still on the device: the result arrays of a call are complete when the NEXT sh_*_batch / sh_*_batch_async call on the context
 * returns (it copies them back after queueing its own first chunk, so the device never idles between calls), or after sh_wait(ctx).
 * The caller keeps the result arrays alive until then.  Results are bit-identical to the synchronous calls. */
int sh_lmm_batch_async(sh_ctx *ctx, const uint8_t *bits, int64_t row_bytes, int64_t V,
                       double *prep, double *pvalue, double *beta, double *bse, double *frac_h2, uint32_t *flags);
int sh_wait(sh_ctx *ctx);
/* Announce the rows of the batch AFTER the next one: called before batch k with the `bits` of batch k+1 (same row_bytes), it lets batch k's
 * copy thread upload the first chunk of batch k+1 while batch k's last chunk runs, so that batch k+1 starts on the device at once (the
 * fixed-effects launch code blocks on its read-backs: without the announcement every call exposes its first upload, 2.8 of 12 ms per 262 144
 * rows).  `bits` must stay valid AND UNCHANGED until batch k+1 has been called with exactly this pointer (the rows may be uploaded at any
 * time in between; the call only probes two 4 KiB windows of them before it trusts the early upload); a batch called with other rows
 * ignores the announcement, and so does anything after sh_*_setup or sh_set_stream.  Optional; results do not depend on it. */
int sh_prefetch_rows(sh_ctx *ctx, const uint8_t *bits, int64_t row_bytes, int64_t V);
/* device-resident variant: d_bits (V*row_bytes bytes), d_out (5*V doubles, SoA in the order above), d_flags (V). */
int sh_lmm_batch_dev(sh_ctx *ctx, const void *d_bits, int64_t row_bytes, int64_t V, void *d_out, void *d_flags);
/* introspection for tests/benchmarks: dominant-kernel work of the last batch */
int sh_lmm_info(sh_ctx *ctx, int *n_limbs, int64_t *int8_macs_per_variant, double *quant_scale);
/* Accuracy of the fixed-point contraction that replaces the reference's fp64 U.T.dot(A) (pyseer/fastlmm/lmm_cov.py:186-193) and
 * computeAKA (:885-900).  The kernel matrix G is held as n_limbs int8 limbs; the only error of x^T K^-1 x is that quantisation, and for a
 * stored row with m' carriers it is bounded by err_norm * ulp * m', err_norm = an upper bound on the spectral norm of the (symmetrised)
 * quantisation error in units of ulp, certified at set-up (sh_lmm_bound_estimate below).  A variant whose relative bound err_norm*ulp*m'/xKx exceeds `tol`
 * (default 1e-8, sh_set_lmm_tol; 0 = never) is contracted again with `extra_limbs` more limbs (up to 56 bits in all = fp64) inside the
 * same call.  bound_typical: the bound of a variant carried by half of the samples on an unstructured population; bound_max_last /
 * refined_last: the largest final bound and the number of re-contracted variants of the LAST batch (synchronises the stream). */
int sh_set_lmm_tol(sh_ctx *ctx, double tol);
int sh_lmm_bound(sh_ctx *ctx, double *err_norm_ulp, double *ulp, double *tol, int *extra_limbs, double *bound_typical,
                 double *bound_max_last, int64_t *refined_last);
/* err_norm (sh_lmm_bound) is a CERTIFIED upper bound since round 3: |E|_2 <= trace(E^(2p))^(1/(2p)) with 2p = 2^(squarings+1), E^(2p) by repeated
 * squaring on the fp64 matrix pipe (64th power at n <= 16384: within 4.4 % of the norm for a Wigner-like error matrix).  The power iteration of
 * rounds 1-2 (which approaches the norm from below and can stall between near-equal or opposite eigenvalues) remains as the estimate reported here.
 * The reference needs neither: it contracts in fp64 (pyseer/fastlmm/lmm_cov.py:186-193, 885-900). */
int sh_lmm_bound_estimate(sh_ctx *ctx, double *power_iteration_ulp, int *squarings);
/* The two norm routines of sh_lmm_setup on a caller-supplied symmetric n x n fp32 matrix (row-major): diagnostic / test entry. */
int sh_spectral_bound_f32(sh_ctx *ctx, const float *A, int n, int squarings, double *upper, double *power_iteration);

/* ---------------------------------------------------------------------------------------------
 * Fixed effects (replaces pyseer/model.py:202 fixed_effects_regression = a1 prefilter + statsmodels Logit newton /
 * OLS + model.py:414 fit_firth).  y: n; W: n x q row-major = [m | c] (MDS components then covariates, no
 * intercept, no variant column; model.py:274-297); null_llf / null_firth from fit_null (model.py:73-148).
 * force_firth != 0 sends every variant through fit_firth (benchmark config C4).
 * ------------------------------------------------------------------------------------------- */
int sh_glm_setup(sh_ctx *ctx, const double *y, const double *W, int q, int continuous,
                 double null_llf, double null_firth, double pret, double lrtt, int force_firth);
/* outputs: prep, pvalue, kbeta, bse, intercept (V each), betas (V*q row-major), flags (V) */
int sh_glm_batch(sh_ctx *ctx, const uint8_t *bits, int64_t row_bytes, int64_t V,
                 double *prep, double *pvalue, double *kbeta, double *bse, double *intercept,
                 double *betas, uint32_t *flags);
/* pipelined form: see sh_lmm_batch_async */
int sh_glm_batch_async(sh_ctx *ctx, const uint8_t *bits, int64_t row_bytes, int64_t V,
                       double *prep, double *pvalue, double *kbeta, double *bse, double *intercept, double *betas, uint32_t *flags);
/* d_out: (5+q)*V doubles SoA: prep,pvalue,kbeta,bse,intercept,betas[0..q) ; d_flags: V.
 * Device memory: the context keeps per-variant workspaces sized for the largest batch seen (logistic with 1..14 covariates:
 * (3(q+2) + 1.5 (q+2)(q+3)/2 + 6) x 8 bytes per variant, 0.9 GB for 2^20 variants at q = 10); sh_glm_batch cuts host batches into
 * 2^18-variant chunks.  A variant's result does not depend on what else is in its batch or on the batch size. */
int sh_glm_batch_dev(sh_ctx *ctx, const void *d_bits, int64_t row_bytes, int64_t V, void *d_out, void *d_flags);
/* The same batch on one of the context's LANES (csrc/lanes_api.inc; the counterpart of the reference's pool of `--cpu N` workers over
 * blocks of variants, pyseer/__main__.py:541-568): a lane is a worker thread with its own stream and per-batch workspaces, set up from the
 * arguments sh_glm_setup was called with.  The call records an event on the context's stream (the rows are ready there), hands the batch to
 * the next free lane and returns; batches of consecutive calls run side by side on the device (one stream of fixed-effects batches leaves it
 * idle between its per-variant kernels and behind the list-length read-backs of its launch code).  d_out / d_flags of a call are complete
 * after sh_wait(ctx) -- which also reports the first error of a lane -- and bit-identical to sh_glm_batch_dev's (a batch is still one
 * sh_glm_batch_dev on one stream).  At most 2 x lanes batches are accepted before the call blocks.  sh_set_lanes: 1..8, default 3; changing
 * it waits for the lanes and tears them down (they are created at the next use).  The job stream (sh_job_*) of a fixed-effects model
 * computes its blocks on the lanes too. */
int sh_glm_batch_dev_async(sh_ctx *ctx, const void *d_bits, int64_t row_bytes, int64_t V, void *d_out, void *d_flags);
int sh_set_lanes(sh_ctx *ctx, int n);
int sh_get_lanes(sh_ctx *ctx);

/* ---------------------------------------------------------------------------------------------
 * Lineage effect (replaces pyseer/model.py:151 fit_lineage_effect): logistic regression of each VARIANT on
 * [1, lin, cov]; lin: n x l row-major (MDS components or cluster indicators, pyseer/__main__.py:417-432), cov: n x j
 * (or NULL, j = 0).  max_lineage[v] = argmax_j |beta_j|/bse_j over the l lineage columns, -1 = None (separation or
 * singular, model.py:193-197).  1 + l + j <= 50 through the dense kernels (registers up to 16, run-time width above).  A design of
 * cluster indicators and nothing else -- j = 0, every entry of lin exactly 0 or 1, at most one 1 per row, at least one row without
 * (the reference cluster, whose column the command line dropped) -- needs no dense Hessian: the count kernel fits it from each
 * cluster's carrier count, for any l up to 1023 (an empty column is legal: every variant answers -1, as the reference does).  It runs
 * where the dense kernels stop (1 + l > 50); SEERHIP_ROUTE lin_counts=1 takes every such design through it, lin_counts=0 none.  Wider
 * designs with covariates or with columns that are not cluster indicators are refused, and the message says which.
 * ------------------------------------------------------------------------------------------- */
int sh_lineage_setup(sh_ctx *ctx, const double *lin, int l, const double *cov, int j);
int sh_lineage_batch(sh_ctx *ctx, const uint8_t *bits, int64_t row_bytes, int64_t V, int32_t *max_lineage);

/* ---------------------------------------------------------------------------------------------
 * Similarity (kinship) matrix from variant presence: replaces pyseer/similarity.py:99-113 (G assembled from
 * load_var_block, pyseer/input.py:678-707, then np.matmul(G, G.T)).  K[i][j] = number of variants carried by both
 * samples among those passing sh_set_af_filter (filtered variants are all-zero columns in the reference, input.py:690-697).
 * sh_sim_begin zeroes the accumulator; accumulate any number of batches (host or device rows, same packed layout as
 * sh_lmm_batch); sh_sim_finish writes the dense N*N row-major fp64 matrix (exact integers) to host memory.
 * --------------------------------------------------------------------------------------------- */
int sh_sim_begin(sh_ctx *ctx);
int sh_sim_accumulate(sh_ctx *ctx, const uint8_t *bits, int64_t row_bytes, int64_t V);
int sh_sim_accumulate_dev(sh_ctx *ctx, const void *d_bits, int64_t row_bytes, int64_t V);
int sh_sim_finish(sh_ctx *ctx, double *K);
/* The matrix as the text the reference prints: pd.DataFrame(K, index=names, columns=names).to_csv(sep='\t') (pyseer/similarity.py:116), made
 * on the device (csrc/simtext_kernels.hip k_sim_text_len, k_sim_format).  K == NULL: the accumulated matrix of sh_sim_begin/accumulate; else a
 * host N x N row-major matrix, which is uploaded.  names + names_off[j] .. names_off[j + 1]: the name of sample j (N + 1 offsets, UTF-8 bytes as
 * they are printed; a name with a tab, a double quote or a line end is refused: the reference's writer would quote it).  nan_mask (NULL: none):
 * N bytes; every cell in the row or the column of a flagged sample is an empty field, as a NaN is.  A header line (an empty first field, the
 * names), one line per sample (its name, then every value as its decimal integer and ".0"), tab-separated, "\n" line ends.
 * *len is always set to the text's length; the text is written only where out != NULL and cap >= *len (out == NULL or a smaller cap: the
 * length query, SH_OK, nothing written).  Lengths and offsets are 64-bit.  A value the notation cannot express -- a non-integer (or a NaN
 * outside nan_mask), a negative (-0.0 too), anything >= 1e15 -- is refused with SH_EINVAL and sh_last_error names the case. */
int sh_sim_text(sh_ctx *ctx, const double *K, const char *names, const int64_t *names_off, const uint8_t *nan_mask, uint8_t *out, int64_t cap,
                int64_t *len);

/* ---------------------------------------------------------------------------------------------
 * Native k-mer text reader / packer (host code; replaces the k-mer branch of pyseer/input.py:301 read_variant for the GPU
 * feed).  Lines "KMER | sample:count sample:count ..." (gzip or plain) -> packed presence rows over `sample_names`
 * (= p.index, phenotype order), carrier counts (af = count / n, input.py:446) and the variant names.
 * ------------------------------------------------------------------------------------------- */
typedef struct sh_reader sh_reader;
sh_reader  *sh_reader_open(const char *path, const char *const *sample_names, int n_samples);
void        sh_reader_close(sh_reader *r);
const char *sh_reader_error(void);
/* how many readers the caller is about to run at once (`--kmers a.gz b.gz ...` = one per file, pyseer/__main__.py:526 reads ONE): readers
 * opened afterwards share the usable CPUs (cgroup quota) between them instead of starting a full worker pool each.  Process-wide hint. */
void        sh_reader_set_concurrency(int n_readers);
/* parses up to max_variants lines; returns how many (0 = end of file, -1 = error, -2 = the variant names of this block need more
 * than names_cap bytes: nothing was consumed, sh_reader_names_needed() gives the size to retry with -- the reference has no limit on
 * name length, and unitig names run to tens of kilobases).  bits: max_variants*row_bytes;
 * names: concatenated variant names, name_off[v] .. name_off[v+1] (max_variants+1 offsets). */
int64_t     sh_reader_next(sh_reader *r, int64_t max_variants, uint8_t *bits, int64_t row_bytes, int32_t *counts,
                           char *names, int64_t names_cap, int64_t *name_off);
int64_t     sh_reader_names_needed(sh_reader *r);
/* bytes of inflated text currently buffered (bounded by one block of lines + one read slab; for tests) */
int64_t     sh_reader_buffered(sh_reader *r);
/* gzip members decoded on several threads (csrc/inflate_par.h): chunks accepted so far that started from a SEARCHED block head (0: the
 * stream was decoded by one thread -- small file, stored/fixed blocks only, SEERHIP_ROUTE reader=serial, BGZF, plain text). */
int64_t     sh_reader_par_chunks(sh_reader *r);
/* The device route of the same reader: containers, inflate, CRC, line framing, names and the -2 accounting stay on the host as above; the
 * sample tokens of every line are read on the device (k_kmer_pack, csrc/kmer_kernels.hip).  The decoder writes its text into pinned slabs,
 * each slab goes to the device once on a stream of the reader's own (never the context's), a call sends one line table and brings the rows
 * and counts back.  A reader opened this way answers sh_reader_next / _names_needed / _buffered / _par_chunks / _close / _error exactly as
 * one from sh_reader_open does.  ctx: its N must be n_samples; NULL selects the kernel's rule restated in plain C++ (host_kmer_pack,
 * csrc/kmer_kernels.h -- another code path than sh_reader_open's parser).  Refuses (NULL, sh_reader_error and sh_last_error) a sample
 * count whose row does not fit the kernel's LDS.
 * sh_reader_dev_stats: lines tokenised by the kernel / by the host restatement (a line longer than the pad that straddles two slabs, every
 * line without a context), text bytes sent to the device, kernel launches.  sh_reader_dev_kernel_ms: the kernel's own time so far (events). */
sh_reader  *sh_reader_open_dev(sh_ctx *ctx, const char *path, const char *const *sample_names, int n_samples);
int         sh_reader_dev_stats(sh_reader *r, int64_t *lines_dev, int64_t *lines_host, int64_t *bytes_up, int64_t *launches);
double      sh_reader_dev_kernel_ms(sh_reader *r);
/* Device inflate (csrc/inflate_dev.h, csrc/inflate_kernels.hip, csrc/inflate_api.inc).  Under SEERHIP_ROUTE kmer_inflate=1 a reader from
 * sh_reader_open_dev has the members of a BGZF file decoded by k_bgzf_inflate, one launch per slab: the compressed bytes go up, the text
 * comes back into the pinned slab for the host's CRC-32, newline index and names, and stays on the device for k_kmer_pack.  A member whose
 * status, length or CRC-32 is wrong afterwards is decoded again on the host; errors read as on the host route.  Other containers are read
 * as without the key.
 * sh_inflate_host: one raw-DEFLATE member by the host build of the kernel's decoder: [cdata, cdata + clen) into [out, out + isize).
 * Returns 0, a positive ShInfStatus of csrc/inflate_dev.h (malformed input; nothing outside either range was touched), or SH_EINVAL.
 * sh_inflate_members_dev: n members through the kernel in one launch, host memory in and out.  Member i is comp[coff[i] .. + clen[i]) and
 * decodes to out[ooff[i] .. + isize[i]) (isize <= 65536); `out` goes up as it is and comes back with min(produced, isize) bytes of every
 * member written and no other byte changed.  status[i], produced[i] as sh_inflate_host gives them; kernel_ms (may be NULL): the kernel's
 * time by stream events.
 * sh_reader_dev_inflate_stats: members decoded by the kernel (without a context: by the host build) / decoded again by the host decoder,
 * bytes sent up (compressed members and their table) and brought back (text and statuses), the kernel's time so far.  All zero where the
 * key is not set or the file is not BGZF.
 * sh_reader_set_inflate: what the calling thread's NEXT sh_reader_open_dev does, whatever the route key says: 1 the device inflate, 0 not,
 * negative as the key says (the state after every open).  Thread-local, so that a caller need not touch the environment. */
void        sh_reader_set_inflate(int on);
int         sh_inflate_host(const uint8_t *cdata, int64_t clen, uint8_t *out, int64_t isize, int64_t *produced);
int         sh_inflate_members_dev(sh_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, const int64_t *coff, const int32_t *clen, const int32_t *isize,
                                   const int64_t *ooff, int64_t n, uint8_t *out, int64_t out_bytes, int32_t *status, int32_t *produced, double *kernel_ms);
int         sh_reader_dev_inflate_stats(sh_reader *r, int64_t *members_dev, int64_t *members_host, int64_t *bytes_up, int64_t *bytes_down, double *kernel_ms);

/* introspection: how many variants of the LAST batch went through the Firth kernel / its pinv slow path */
int sh_glm_info(sh_ctx *ctx, int64_t *firth_routed, int64_t *pinv_routed);

/* ---------------------------------------------------------------------------------------------
 * Result sink: array-backed results -> the reference's TSV rows (pyseer/utils.py:39-105 format_output, the print loop of
 * pyseer/__main__.py:805-827).  CPU only.  For every selected row v = sel[r], in order:
 *   name \t cols[0][v] \t ... \t cols[ncol-1][v] [\t betas[v*q .. v*q+q) if betas_valid[v]] [\t label | NA] \t notes \n
 * numbers as '%.2E', non-finite -> empty field; notes = names of flag bits 0..8 joined by ','.
 * names/name_off: concatenated variant names as sh_reader_next delivers them.  lineage may be NULL (no column).
 * Returns the number of bytes written, or -(needed+1) when cap is too small (nothing written), -1 on bad arguments.
 * Formatting runs on the calling thread and the idle workers of the process-wide host pool; any number of threads may call at once
 * (each owns its text buffers: no lock).
 * --------------------------------------------------------------------------------------------- */
int64_t sh_format_rows(const char *names, const int64_t *name_off, const int64_t *sel, int64_t nsel,
                       const double *const *cols, int ncol, const double *betas, int q, const uint8_t *betas_valid,
                       const int32_t *lineage, const char *const *lineage_labels, int n_labels,
                       const uint32_t *flags, char *out, int64_t cap);


/* ---------------------------------------------------------------------------------------------
 * Job stream (round 5): blocks of a variant stream in, the TSV text of the rows the run PRINTS and the run's counters out.
 * Replaces, per block, the reference's print loops pyseer/__main__.py:571-593 (fixed effects) and :805-827 (LMM) over the tuples of
 * fixed_effects_regression / fit_lmm, with format_output (pyseer/utils.py:39-105) on the rows that pass: rows that are not pre-filtered and
 * not filtered (or every row with print_filtered, LMM blocks then listing their filtered rows first and NaN-masked as pyseer/lmm.py:160-217
 * leaves them).  Selection, the counters and the compaction of the printed rows' statistics run on the device (csrc/job_kernels.hip); the host
 * formats only printed rows.  The stream is pipelined three blocks deep: sh_job_submit queues the upload of block k and the kernels of block
 * k-1 and returns; sh_job_collect waits (asleep between polls of the block's event) for the OLDEST uncollected block and returns its text, valid until the
 * calling thread's next sh_job_collect / sh_format_* call.  At most sh_job_depth(job) blocks may be submitted and not yet collected.
 *   bits/row_bytes/V: as sh_lmm_batch;  counts[v]: carriers of variant v (af = counts / n_samples, pyseer/input.py:446);
 *   names/name_off: concatenated variant names as sh_reader_next delivers them.  All four must stay valid until the block is collected.
 *   rows_are_dma != 0: `bits` lies in pinned or registered host memory (sh_host_register) and is read by the device where it lies;
 *   otherwise the rows are copied through a pinned slab by the calling thread and the process-wide host pool.
 *   counters[0..2] of sh_job_collect: pre-filtered, tested, printed variants of the block (the reference's stderr summary, __main__.py:595-599).
 * sh_job_set_lineage (round 6; before the first block): fit_lineage_effect (pyseer/model.py:151-199) inside the stream, on the design of
 *   sh_lineage_setup, for the rows the run PRINTS, its label (labels[index], or NA) in the reference's column (pyseer/utils.py:88-95).  Fixed
 *   effects: every printed row the reference reaches the fit with (model.py:379-382: not pre-filtered, no firth-fail).  LMM: ONE fit per block
 *   -- of the block's LAST variant -- given to every row that passed, which is what pyseer/lmm.py:209-213 computes (it calls the fit with the
 *   stale `k` of its loading loop), so blocks must be the reference's (--block_size); per_variant != 0 fits each passing row's own variant.
 * sh_job_set_patterns (--output-patterns): hash_pattern (pyseer/input.py:710-723) -- base64(md5(the presence vector as int64)) + "\n" -- of every
 *   TESTED variant of a block (not pre-filtered; print loops pyseer/__main__.py:584-585, 794-795, 818-819), computed on the device (one lane
 *   per variant; the md5 of 8 N bytes is 60 us of a CPU core per variant at N = 5000); sh_job_patterns returns the text of the block last
 *   collected (25 bytes per tested variant, in input order), valid until the next sh_job_collect.
 * sh_job_set_samples (--print-samples): the two sample lists of pyseer/utils.py:96-98 (carriers, then the others, comma-joined) in front of
 *   the notes of every PRINTED row, read from the row's bits on the host: names / name_off = the n_samples sample names (concatenated, n + 1
 *   offsets) in the context's sample order, order[i] = the sample printed i-th (the reference sorts the names).
 * --------------------------------------------------------------------------------------------- */
typedef struct sh_job sh_job;
sh_job *sh_job_open(sh_ctx *ctx, int lmm, int print_filtered);
void    sh_job_close(sh_job *job);
int     sh_job_submit(sh_job *job, const uint8_t *bits, int64_t row_bytes, int64_t V, const int32_t *counts,
                      const char *names, const int64_t *name_off, int rows_are_dma);
/* sh_job_submit_calls (round 20): a block of CALLS as the native VCF / Rtab readers deliver them (sh_vcf_next, sh_burden_fold, sh_rtab_next) -- per record
 * the packed `present` and `missing` planes (row_bytes each), their popcounts and the reader's skip reason -- instead of rows that hold no missing call.
 * Lifetime and depth rules of sh_job_submit: everything pointed at stays valid until the block has been collected.  Per row, after the batch's own
 * fan-out (k_job_calls_mark):
 *   skip != 0                      counted as pre-filtered, never a row of the output (not with print_filtered either), no pattern;
 *   af = (n_present + n_missing) / n_samples outside the context's AF window (sh_set_af_filter, inclusive), or n_missing / n_samples > max_missing
 *                                  af-filter, pre-filtered, every statistic NaN (af itself is printed);
 *   n_missing == 0                 fitted from `present`, exactly as a row of sh_job_submit;
 *   n_missing > 0                  pre_filtering (pyseer/model.py:31-70) over the samples that have a call; `pre-filtering-failed` where it fails or is
 *                                  not finite, else filtered with `missing-data-error` (fixed effects, model.py:371-377) or `lrt-filtering-failed` (LMM,
 *                                  lmm.py:190-204); every statistic but filter-pvalue NaN, lineage NA.
 * Patterns (sh_job_set_patterns, sh_job_set_pattern_count): a row with a missing call is hashed as the float64 vector with NaN that the reference
 * hashes (k_job_md5_calls) and enters the pattern set as that digest.  sh_job_set_samples: the carriers are present | missing.  The LMM's per-block
 * lineage (sh_job_set_lineage, per_variant = 0) is none where the block's last record was skipped or holds a missing call. */
int     sh_job_submit_calls(sh_job *job, const uint8_t *present, const uint8_t *missing, int64_t row_bytes, int64_t V, const int32_t *n_present,
                            const int32_t *n_missing, const int32_t *skip, const char *names, const int64_t *name_off, double max_missing);
int     sh_job_collect(sh_job *job, const char **text, int64_t *nbytes, int64_t *counters);
/* the records the text of the block last collected was formatted from, as the device compacted them: idx[r] = the row's index in its block,
 * flags[r], cols[a * stride + r] = statistic a (filter-pvalue, lrt-pvalue, beta, beta-std-err, intercept / variant_h2, then the covariate
 * slopes; NaN-masked as printed), r < nsel.  Valid until the next sh_job_submit / sh_job_submit_calls. */
int     sh_job_records(sh_job *job, int64_t *nsel, const int32_t **idx, const uint32_t **flags, const double **cols, int64_t *stride, int *nrow);
/* measurement (tools/calls_job_bench.py): stream events around k_job_calls_mark and, in a job that counts patterns without writing them, k_job_md5_calls
 * of every later call block; sh_job_calls_times waits for them and returns their sums in ms and their numbers, and starts the record again.
 * Both with no block in flight. */
int     sh_job_set_calls_timing(sh_job *job, int on);
int     sh_job_calls_times(sh_job *job, double *mark_ms, int64_t *mark_launches, double *md5_ms, int64_t *md5_launches);
int64_t sh_job_pending(sh_job *job);
int     sh_job_depth(sh_job *job);     /* blocks that may be submitted and not yet collected: 3 (LMM), 2 + lanes (fixed effects) */
int     sh_job_set_lineage(sh_job *job, const char *const *labels, int n_labels, int per_variant);
int     sh_job_set_patterns(sh_job *job, int on);
int     sh_job_patterns(sh_job *job, const char **text, int64_t *nbytes);
int     sh_job_set_pattern_count(sh_job *job, int on);   /* the job's context must have a set begun: the pattern set below */
int     sh_job_set_samples(sh_job *job, const char *names, const int64_t *name_off, const int32_t *order, int n);
/* The whole block loop of one stream of a packed cache (pyseer_amd/input.py PackedCacheWriter: the `--save-packed` / `--load-packed` file) in
 * one call -- the loop over load_var_block / fit / print of pyseer/__main__.py:541-593, 777-827 for part `part_i` of `part_n` contiguous ranges
 * of the cache's rows (the reference's `--cpu N`; one part per device).  Stored blocks are merged to at least block_rows rows (never split)
 * exactly as the single stream would cut them; rows go to the device by DMA from registered windows of the file's mapping (use_dma != 0; a
 * block merged from several stored blocks range by range, each to its place) or through pinned slabs; the text of the printed rows is written to out_fd, the pattern text (sh_job_set_patterns) to pat_fd, in input order.
 * counters[0..3] += pre-filtered, tested, printed variants and blocks.  *stop != 0 (may be NULL) ends the stream at the next block.  The
 * calling thread holds no interpreter lock: streams of several contexts run side by side on threads of one process. */
int     sh_job_run_packed(sh_job *job, const char *path, int part_i, int part_n, int64_t block_rows, int use_dma, int out_fd, int pat_fd,
                          int64_t *counters, const volatile int *stop);
/* the formatter behind sh_job_collect, callable on its own (tests): nsel compacted records -- idx[r] = the variant's index into names / counts,
 * flags[r], cols[c][r] (c < ncol), slopes betas[j * betas_stride + r] printed where betas_valid[r] -- as
 *   name \t counts[idx]/n_samples \t cols... [\t betas...] [\t lineage label] \t notes \n ; lineage[r] = index into lineage_labels or -1 (NA), NULL =
 *   no lineage column; *text is owned by the calling thread (valid until its next call). */
int64_t sh_format_records(const char *names, const int64_t *name_off, const int32_t *counts, int n_samples, const int32_t *idx, int64_t nsel,
                          const double *const *cols, int ncol, const double *betas, int64_t betas_stride, int q, const uint8_t *betas_valid,
                          const int32_t *lineage, const char *const *lineage_labels, int n_labels, const uint32_t *flags, const char **text);
/* Make [p, p + nbytes) (e.g. a window of a read-only file mapping: the packed cache) readable by the device where it lies, so that the rows
 * cross PCIe by DMA with no CPU copy (hipHostRegister on the enclosing pages; measured 4 ns of CPU per 632-byte row against 21 for the
 * copy into pinned staging, profiles/r05/host_feed_probe.txt).  `device`: the device whose stream will read it (the registration itself is portable).
 * Unregister with the same p once the rows have been collected. */
int     sh_host_register(const void *p, int64_t nbytes, int device);
int     sh_host_unregister(const void *p);
/* The host CPU budget (csrc/host_pool.h): every host-side helper of this library -- readers, the stager of pageable rows, the formatter --
 * draws on ONE persistent pool sized to the CPUs the process may use (affinity mask cut by the cgroup quota), the counterpart of the
 * reference's `--cpu N`.  sh_set_host_threads overrides the detected number (0 = detect); sh_set_host_streams says how many device streams
 * (or readers) the caller runs at once, so per-stream helpers take their share (generalises sh_reader_set_concurrency).
 * sh_host_cpu_seconds: thread CPU seconds spent per host stage so far ("stage=seconds,..."); returns the length, or -(needed+1). */
int     sh_host_cpus(void);
void    sh_set_host_threads(int n);
void    sh_set_host_streams(int n);
int     sh_host_pool_workers(void);
int     sh_host_cpu_seconds(char *buf, int cap);
/* the largest number of threads that were inside sh_format_rows / sh_format_records at the same time (reset != 0 clears it): tests */
int     sh_format_concurrency_max(int reset);

/* ---------------------------------------------------------------------------------------------
 * The run-wide set of distinct presence patterns (--count-patterns).  Replaces scripts/count_patterns.py of the reference, which takes
 * the file --output-patterns wrote (one base64 md5 line per tested variant, pyseer/input.py:710-723), runs `LC_ALL=C sort -u | wc -l`
 * over it and prints the Bonferroni threshold alpha / count.  Two variants have the same md5 exactly when their presence rows are equal, so
 * the count is the number of distinct packed rows: the set keeps one 128-bit key per row (two independently seeded 64-bit sums over the
 * row's 64-bit words and their indices, the N sample bits only; n distinct rows collide with probability about n^2 / 2^129, the order of
 * md5's own) in an open-addressing table in device memory that lives across the blocks of a run and doubles before its load passes 1/2.
 * No md5, no text, no sort.
 *   begin: initial_slots 0 = 2^20, else a power of two >= 1024.  One set per context, until end (or sh_destroy).
 *   add_rows: V host rows as sh_lmm_batch takes them, every row inserted; add_rows_dev: the same rows in device memory.
 *   add_keys: n ready-made keys of two 64-bit words each, e.g. the 16 bytes of an md5 digest made on the host (rows with missing calls
 *     never reach the device).  A half equal to ~0 is stored as 0: (~0, b) and (0, b) count as one key, and so do (a, ~0) and (a, 0).
 *   count: waits for the inserts queued so far (the lanes' included); distinct keys, the table's slots, how often it grew.
 *   hash_rows: the keys the device gives the same rows (2 V words), on the host, no context: add_keys of them equals add_rows.
 * A job with sh_job_set_pattern_count on inserts the rows sh_job_set_patterns would digest -- every TESTED row of a block -- on the stream of
 * the block's own kernels, with or without sh_job_set_patterns.  Inserts and counts are asynchronous to the caller except where stated.
 * ------------------------------------------------------------------------------------------- */
int     sh_patset_begin(sh_ctx *ctx, int64_t initial_slots);
int     sh_patset_add_rows(sh_ctx *ctx, const uint8_t *bits, int64_t row_bytes, int64_t V);
int     sh_patset_add_rows_dev(sh_ctx *ctx, const void *d_bits, int64_t row_bytes, int64_t V);
int     sh_patset_add_keys(sh_ctx *ctx, const uint64_t *keys, int64_t n);
int     sh_patset_count(sh_ctx *ctx, int64_t *distinct, int64_t *slots, int64_t *growths);
int     sh_patset_end(sh_ctx *ctx);
int     sh_patset_hash_rows(const uint8_t *bits, int64_t row_bytes, int64_t V, int n_samples, uint64_t *keys);

/* ---------------------------------------------------------------------------------------------
 * Native VCF reader (csrc/vcf_reader.cpp + csrc/vcf_kernels.hip; replaces the 'vcf' branch of pyseer/input.py:301 read_variant and
 * read_vcf_var, input.py:455-503, for the GPU feed).  VCF text -- plain, gzip or BGZF; no index file is read -- is decoded, framed and
 * its nine fixed columns parsed on the host; the sample columns go to the device as they stand and k_vcf_gt_pack reduces every sample's
 * GT to present / missing / absent.  Bound to a context because it uses its device and stream; ctx == NULL selects the host restatement of
 * the kernel (measurements, and checks where there is no device) -- the command line never passes NULL.
 * BCF 2.1 / 2.2 comes through the same entry points: the decoded stream is sniffed ("BCF\2"), records are framed by their length words,
 * the shared block gives the name, the skip reason, POS and len(REF), and only the GT vector (n_sample x L bytes; int16 / int32 narrowed
 * on the host) goes to the device, where k_bcf_gt_pack reduces it by the same rule.  BCF1 and minor versions above 2 are refused.
 *   sh_vcf_next: up to max_records records -> per record the skip reason (0 kept, 1 more than one ALT, 2 FILTER neither empty nor PASS;
 *   skipped records have rows of zeros), POS, len(REF), the contig's id (sh_vcf_contig), and two packed rows over sample_names in the
 *   engine's layout (LSB first, row_bytes as sh_lmm_batch): `present` and `missing` (a sample is never in both) with their popcounts.
 *   Returns the number of records, 0 at the end of the file, -1 on error (sh_last_error).
 *   sh_vcf_names: the names CHROM_POS_REF[_ALT] of the LAST sh_vcf_next as one blob + offsets (layout of sh_reader_next), owned by the
 *   reader and valid until its next call; returns the blob's length.
 *   sh_burden_fold: burden variant v = records csr_idx[csr_off[v] .. csr_off[v+1]) of a batch of rows, in application order: present =
 *   OR of their present rows, missing = the LAST record's missing row where not present (input.py:383-407); host pointers.
 * ------------------------------------------------------------------------------------------- */
typedef struct sh_vcf sh_vcf;
sh_vcf     *sh_vcf_open(sh_ctx *ctx, const char *path, const char *const *sample_names, int n_samples);
void        sh_vcf_close(sh_vcf *r);
int64_t     sh_vcf_next(sh_vcf *r, int64_t max_records, int32_t *skip, int64_t *pos, int32_t *ref_len, int32_t *contig, uint8_t *present, uint8_t *missing,
                        int64_t row_bytes, int32_t *n_present, int32_t *n_missing);
int64_t     sh_vcf_names(sh_vcf *r, const char **blob, const int64_t **name_off);
/* mode: 0 plain, 1 gzip, 2 BGZF; the sample columns of the header; contigs met so far */
int         sh_vcf_info(sh_vcf *r, int *mode, int *n_cols, int *n_contigs);
/* what the decoded bytes hold: 0 VCF text, 1 BCF (sniffed when the file is opened, whatever its name) */
int         sh_vcf_format(sh_vcf *r);
const char *sh_vcf_contig(sh_vcf *r, int id);
/* bytes of sample columns handed to the tokeniser, records delivered, kernel launches so far */
int         sh_vcf_stats(sh_vcf *r, int64_t *sample_bytes, int64_t *records, int64_t *launches);
int         sh_burden_fold(sh_ctx *ctx, const uint8_t *present, const uint8_t *missing, int64_t row_bytes, int64_t n_records, const int64_t *csr_off,
                           const int32_t *csr_idx, int64_t n_variants, uint8_t *out_present, uint8_t *out_missing, int32_t *n_present, int32_t *n_missing);

/* ---------------------------------------------------------------------------------------------
 * Native Rtab reader (csrc/rtab_reader.cpp + csrc/rtab_kernels.hip; replaces the 'Rtab' branch of pyseer/input.py:301 read_variant for the
 * GPU feed).  A presence/absence table -- plain text, as roary, panaroo, piggy or `unitig-caller --rtab` write it -- is framed on the host
 * exactly as Python's text mode frames it (\n, \r\n, a lone \r; a last line without terminator), every line stripped at its end of what
 * str.rstrip() strips among ASCII bytes, and split at its first tab into the name and the call text; the call text goes to the device as it
 * stands and k_rtab_pack reduces every call to present (`1`) / missing (`.` or empty) / absent (`0`).  Bound to a context because it uses
 * its device and stream; ctx == NULL selects the host restatement of the kernel (measurements, and checks where there is no device).
 *   sh_rtab_open: `columns` are the sample columns of the header as the caller split them (the reference: header.rstrip().split()[1:]); the
 *   reader skips the file's first line and does not parse it.  A column that names no sample is ignored; a sample without a column is absent
 *   in every row.  A sample named by two columns is refused -- the reference lets the last call that is not `0` win, which OR-ing bits cannot
 *   give -- with a message that begins "Rtab: duplicate sample column": the caller then reads the table line by line.
 *   sh_rtab_next: up to max_rows lines -> per line a status and two packed rows over sample_names in the engine's layout (LSB first,
 *   row_bytes as sh_lmm_batch): `present` and `missing` (a sample is never in both) with their popcounts.  status: 0 ok; 1 the line has no
 *   calls ("No sample data found; is this a Rtab file?"); 2 the number of calls is not the header's ("Unexpected mismatch between header
 *   and data row"); 3 a call that is none of `0`, `1`, `.`, empty, in any column ("Rtab file not binary") -- in this order of precedence,
 *   the reference's.  A malformed line is a status and not an error, because a caller that selects lines by name passes over the others
 *   unchecked; its rows are zeros.  Returns the number of lines, 0 at the end of the file, -1 on an I/O or HIP error (sh_last_error).
 *   sh_rtab_names: the names of the LAST sh_rtab_next (everything before a line's first tab) as one blob + offsets (layout of
 *   sh_reader_next), owned by the reader and valid until its next call; returns the blob's length.
 * ------------------------------------------------------------------------------------------- */
typedef struct sh_rtab sh_rtab;
sh_rtab    *sh_rtab_open(sh_ctx *ctx, const char *path, const char *const *sample_names, int n_samples, const char *const *columns, int n_columns);
void        sh_rtab_close(sh_rtab *r);
int64_t     sh_rtab_next(sh_rtab *r, int64_t max_rows, int32_t *status, uint8_t *present, uint8_t *missing, int64_t row_bytes, int32_t *n_present,
                         int32_t *n_missing);
int64_t     sh_rtab_names(sh_rtab *r, const char **blob, const int64_t **name_off);
/* bytes of call text handed to the tokeniser, lines delivered, kernel launches so far */
int         sh_rtab_stats(sh_rtab *r, int64_t *call_bytes, int64_t *rows, int64_t *launches);
/* how k_rtab_pack divides a line's call text: bytes per lane, per wavefront and per step of all lanes (tests place line ends there) */
int         sh_rtab_partition(sh_rtab *r, int *lane_bytes, int *wave_bytes, int *step_bytes);

/* ---------------------------------------------------------------------------------------------
 * Whole-genome elastic net (csrc/enet_kernels.hip + csrc/enet_api.inc; replaces pyseer/enet.py load_all_vars :33-118, correlation_filter
 * :379-421 and the cvglmnet call of fit_enet :177-185).  One bit matrix of every variant that passed the filters stays on the device; the full
 * fit and each cross-validation fold are that matrix with other sample weights (a held-out sample has weight 0).
 *   begin / append / end: reserve `capacity` rows of row_bytes (layout of sh_lmm_batch), add V rows.  flip[v] != 0 (may be NULL) stores the
 *     row in the minor-allele coding of enet.py:95-106: by its absences, a missing call (the `missing` rows, may be NULL) being 0 either way.
 *   ingest: load_all_vars' loop (enet.py:33-118) for a block of V parsed rows WITHOUT missing calls (k-mers: the native reader's or the packed
 *     cache's raw blocks, every parsed line, host pointer), decided on the device (k_enet_ingest_*): a row is kept iff its carriers over the
 *     first n_samples bits (padding bits are not trusted) lie in [min_count, max_count] -- the caller derives the two from the reference's
 *     strict `af > min_af and af < max_af` evaluated at every count; an empty interval keeps nothing -- and is stored after the rows already
 *     there, in the order of the block, by its absences when 2 * carriers > n_samples (enet.py:95-106).  Returns the number of rows kept
 *     (their index in the block and their carrier count in kept_idx / kept_count, V entries each, the caller's) or a negative status.
 *     The matrix grows as needed (sh_enet_begin's capacity is the initial one: at least twice the rows, copied device to device); a growth
 *     that fails returns SH_ENOMEM with the matrix as it was.  Forgets the last fit, like append.
 *   ingest_calls: the same loop for a block of V parsed rows WITH missing calls (the layout sh_vcf_next and sh_burden_fold write: a present
 *     and a missing row per variant, host pointers; missing may be NULL: no missing calls; skip may be NULL, else skip[v] != 0 drops row v:
 *     the reader's skip reason).  Over the first n_samples bits c = popcount(present), m = popcount(missing & ~present), t = c + m: the
 *     reference counts a missing call as a carrier in af (input.py:439-446).  A row is kept iff it is not skipped, min_count <= t <= max_count
 *     and m <= max_missing_count (an empty interval or max_missing_count < 0 keeps nothing), and is stored by its absences (~present &
 *     ~missing) when 2 * t > n_samples: the words sh_enet_append(present, missing, flip) stores.  kept_idx / kept_present / kept_missing
 *     (V entries each, the caller's) take the block index, c and m of the kept rows; growth, SH_ENOMEM and the last fit as for ingest.
 *     With missing == NULL and skip == NULL it is ingest.
 *   correlations: |cor(row, y)| of enet.py:398-418 for every row, NaN for a row without carriers.  The quantile cut is the caller's.
 *   keep: compact the matrix to rows idx[0 .. n_keep) (ascending or not); get_rows: copy rows idx[] out (host pointer), e.g. the selected
 *     variants for the per-variant engine, so that no input is read twice (enet.py:424 find_enet_selected reads it again).
 *   fit: y, weights (NULL = 1; normalised to sum 1), n_cov dense covariate columns (covariates[k * n_samples + i], penalised like variants,
 *     enet.py:173-174), fold_id[i] in [0, n_folds) (n_folds = 0: no cross-validation), family 0 gaussian / 1 binomial, alpha in [0, 1].
 *     Minimises glmnet's objective with standardize = intercept = TRUE over a path of n_lambda penalties from lambda_max down (DESIGN.md
 *     section 12 states every rule); arrays of sh_enet_out are the caller's, of opts->n_lambda entries (fold_dev: n_folds x n_lambda,
 *     row f at f * opts->n_lambda; beta: n_cov + rows), any may be NULL.  out->n_lambda = values fitted before the path ended,
 *     i_min = argmin cvm (-1 without folds), beta0 / beta = the full fit at i_min (at the last value without folds), original scale.
 *   betas_at: the solution of problem 0 (full fit) or 1 + k (fold k held out) at lambda i of the last fit; eta_at: the full fit's linear
 *     predictor of every sample there.
 * ------------------------------------------------------------------------------------------- */
typedef struct sh_enet_opts {
    int32_t n_lambda;          /* 0 = 100 */
    int32_t max_sweeps;        /* sweeps per launch before the host looks again; 0 = 100000.  A binomial launch that ends on this budget
                                * restarts with a fresh IRLS step, so the 25-step IRLS cap counts per launch and the iterates (not the
                                * optimum) depend on this value: leave it at 0 unless a launch must stay short */
    int32_t state_in_global;   /* != 0: keep the per-sample state in global memory even where it fits the LDS */
    int32_t reserved;
    double  thresh;            /* glmnet's thresh: a solve ends when the largest xv_j delta_j^2 of a sweep < thresh x null deviance; 0 = 1e-7 */
    double  lambda_min_ratio;  /* 0 = glmnet's default: 1e-2 if n_samples < columns else 1e-4 */
    const double *lambda_seq;  /* NULL, or n_lambda decreasing penalties to use instead of the computed sequence (glmnet's `lambda`) */
} sh_enet_opts;
typedef struct sh_enet_out {
    int32_t n_lambda, i_min, kkt_rounds, state_in_lds;
    int64_t cd_sweeps, cd_steps;   /* sweeps and coordinate steps of k_enet_cd, summed over problems */
    double  beta0, cvm_min;
    double *lambda, *cvm, *cvsd, *dev_ratio, *fold_dev, *fold_weight, *beta;
    int32_t *nzero;
} sh_enet_out;
int     sh_enet_begin(sh_ctx *ctx, int64_t row_bytes, int64_t capacity);
int     sh_enet_append(sh_ctx *ctx, const uint8_t *present, const uint8_t *missing, const uint8_t *flip, int64_t V);
int64_t sh_enet_ingest(sh_ctx *ctx, const uint8_t *bits, int64_t V, int32_t min_count, int32_t max_count, int32_t *kept_idx, int32_t *kept_count);
int64_t sh_enet_ingest_calls(sh_ctx *ctx, const uint8_t *present, const uint8_t *missing, const int32_t *skip, int64_t V, int32_t min_count, int32_t max_count,
                             int32_t max_missing_count, int32_t *kept_idx, int32_t *kept_present, int32_t *kept_missing);
int64_t sh_enet_rows(sh_ctx *ctx);
int     sh_enet_correlations(sh_ctx *ctx, const double *y, double *out_abs_cor);
/* out[f * rows + j] = sum over the carriers i of row j of vectors[f * n_samples + i] (k_enet_grad, 16 vectors a pass): the pass behind the
 * weighted means, lambda_max, the strong rule and the KKT check, callable on its own (tests, measurements) */
int     sh_enet_carrier_sums(sh_ctx *ctx, const double *vectors, int n_vectors, double *out);
int     sh_enet_keep(sh_ctx *ctx, const int64_t *idx, int64_t n_keep);
int     sh_enet_get_rows(sh_ctx *ctx, const int64_t *idx, int64_t n, uint8_t *rows);
int     sh_enet_fit(sh_ctx *ctx, const double *y, const double *weights, const double *covariates, int n_cov, const int32_t *fold_id, int n_folds,
                    int family, double alpha, const sh_enet_opts *opts, sh_enet_out *out);
int     sh_enet_betas_at(sh_ctx *ctx, int problem, int i_lambda, double *beta0, double *beta);
int     sh_enet_eta_at(sh_ctx *ctx, int i_lambda, double *eta);
int     sh_enet_end(sh_ctx *ctx);

/* ---------------------------------------------------------------------------------------------
 * Prediction from a saved elastic-net model (csrc/enet_kernels.hip k_enet_predict + csrc/enet_api.inc, csrc/nameset.cpp; replaces the loop
 * of pyseer/enet_predict.py:159-179).
 *   sh_predict_begin: a resident fp64 accumulator of n_samples, initialised from start[n_samples] (the intercept plus the covariate terms,
 *     the caller's).  sh_predict_add: for k = 0 .. n_sel-1 in this order, acc[i] = acc[i] + k_i * beta[k] over every sample i, where k_i is
 *     bit i of row row_idx[k] of the host block `present` (rows of row_bytes, layout of sh_lmm_batch; bits at and above n_samples are not
 *     read as samples), complemented where flip[k] != 0; where `missing` (same shape, may be NULL) has the bit set, k_i is NaN for a row
 *     that is not flipped and 0 for one that is.  The addend is the product, so a zero keeps numpy's sign.  Only the selected rows are
 *     staged and uploaded; row_idx[k] must index a row of the block (the caller's check: the library is not told how many rows it holds).
 *     Every sample's sum is sequential in the order of the calls and of row_idx: the bits of the result do not depend on how the rows are
 *     split over calls.  sh_predict_end: copies the accumulator to link[n_samples] (may be NULL) and frees it.
 *   sh_nameset_*: the model's names (one blob, n + 1 offsets) as a hash set on the host.  match: the rows v of a block's names (blob, V + 1
 *     offsets) whose name is in the set and has not been met before, in block order -> row_idx[], and which name -> model_idx[] (V entries
 *     each, the caller's); returns their number, or -1 for bad arguments.  A name is retired at its first hit (the reference pops it), so a
 *     second line of the same name is not returned.  left: names not met yet.  One thread, no device.
 * ------------------------------------------------------------------------------------------- */
typedef struct sh_nameset sh_nameset;
int         sh_predict_begin(sh_ctx *ctx, const double *start);
int         sh_predict_add(sh_ctx *ctx, const uint8_t *present, const uint8_t *missing, int64_t row_bytes, const int64_t *row_idx, const double *beta,
                           const uint8_t *flip, int64_t n_sel);
int         sh_predict_end(sh_ctx *ctx, double *link);
sh_nameset *sh_nameset_new(const char *blob, const int64_t *off, int64_t n);
int64_t     sh_nameset_match(sh_nameset *set, const char *blob, const int64_t *off, int64_t V, int64_t *row_idx, int32_t *model_idx);
int64_t     sh_nameset_left(const sh_nameset *set);
void        sh_nameset_free(sh_nameset *set);

/* ---------------------------------------------------------------------------------------------
 * A packed cache served to a subset or another order of its samples (csrc/select_kernels.hip k_rows_select + csrc/select_api.inc;
 * pyseer_amd/input.py iter_packed_blocks_cached with `select`).  A cache written over samples S holds every parsed line of the k-mer file;
 * a run over n_dst of them, in any order, sees the same lines with bit j of a row = bit map[j] of the stored row.
 *   open: map[n_dst] (host) names distinct source bits, each in [0, n_src); n_dst must be the context's n_samples.  The table is uploaded;
 *     the selector owns a stream and pinned staging of its own and runs beside the context's job stream and lanes.  NULL on error
 *     (sh_last_error); n_src above what a source row may take of the LDS (64 KB: 524 288 samples) is refused.
 *   rows: V host rows of src_row_bytes (a multiple of 8, at least n_src bits) -> V host rows of ((n_dst + 63) / 64) * 8 bytes, every bit at or
 *     above n_dst zero whatever the source's padding bits hold, and each row's carrier count among the n_dst samples.  Complete when the call
 *     returns.  src_is_dma != 0: `bits` lies in memory the device may read where it is (sh_host_register); out_bits may be any host memory.
 *   rows_dev: the same with rows, output and counts in device memory (8-byte aligned), on the selector's stream; complete at return.
 *   rows_host: the rule restated in plain C++ on the host pool, no context and no device: checks, and the rate to compare against.
 *   sh_sim_accumulate_select: V host rows of the source width into the similarity accumulator of the selector's context (sh_sim_begin has
 *     run): staged through the selector's pinned memory, uploaded and selected on its stream, accumulated on the context's as
 *     sh_sim_accumulate_dev does (sh_set_af_filter applies to the counts over the n_dst samples); the two streams are ordered by events.
 *     Every row crosses to the device once and none comes back.  Complete when the call returns.
 * One thread per selector at a time.
 * ------------------------------------------------------------------------------------------- */
typedef struct sh_select sh_select;
sh_select  *sh_select_open(sh_ctx *ctx, int n_src, const int32_t *map, int n_dst);
void        sh_select_close(sh_select *s);
int         sh_select_rows(sh_select *s, const uint8_t *bits, int64_t src_row_bytes, int64_t V, uint8_t *out_bits, int32_t *out_counts, int src_is_dma);
int         sh_select_rows_dev(sh_select *s, const void *d_bits, int64_t src_row_bytes, int64_t V, void *d_out, int32_t *d_counts);
int         sh_select_rows_host(const uint8_t *bits, int64_t src_row_bytes, int64_t V, int n_src, const int32_t *map, int n_dst, uint8_t *out_bits,
                                int32_t *out_counts);
int         sh_sim_accumulate_select(sh_ctx *ctx, sh_select *sel, const uint8_t *bits, int64_t src_row_bytes, int64_t V);
/* A call cache served the same way (k_calls_select; pyseer_amd/input.py iter_call_cache_blocks): blocks of CALLS hold a present and a missing
 * plane of the same rows, and one pass restricts both -- the map is loaded once for the two.
 *   calls: V host rows of each plane, src_row_bytes wide -> V host rows of each plane over the n_dst samples (pad bits zero) with n_present
 *     and n_missing among them (int32).  Staged through the selector's pinned memory on its stream; complete at return.  A source row wider
 *     than 32 768 bytes (262 144 samples: one wavefront's two planes in 64 KB of LDS) is refused, here and below.
 *   calls_dev: the same for device memory (8-byte aligned); sh_select_kernel_ms: the time between stream events around its last launch.
 *   calls_host: the rule in plain C++ on the host pool, no context and no device.
 *   sh_job_submit_calls_select: sh_job_submit_calls for a block over the selector's n_src samples.  The source planes are uploaded once, through
 *     the selector's pinned memory; k_calls_select writes the selected planes and their counts into the job slot's device buffer; the counts
 *     alone come back (8 bytes a row: the printed af, and whether the LMM's per-block lineage exists), and the selected planes too when the job
 *     lists samples (sh_job_set_samples).  The selector must belong to the job's context; its stream and the job's are ordered by events.
 *     present, missing and skip are the caller's again at return; names and name_off until the block is collected.  Depth and refusals as
 *     sh_job_submit_calls. */
int         sh_select_calls(sh_select *s, const uint8_t *present, const uint8_t *missing, int64_t src_row_bytes, int64_t V, uint8_t *out_present,
                            uint8_t *out_missing, int32_t *out_n_present, int32_t *out_n_missing);
int         sh_select_calls_dev(sh_select *s, const void *d_present, const void *d_missing, int64_t src_row_bytes, int64_t V, void *d_out_present,
                                void *d_out_missing, int32_t *d_n_present, int32_t *d_n_missing);
int         sh_select_kernel_ms(sh_select *s, double *ms);
int         sh_select_calls_host(const uint8_t *present, const uint8_t *missing, int64_t src_row_bytes, int64_t V, int n_src, const int32_t *map, int n_dst,
                                 uint8_t *out_present, uint8_t *out_missing, int32_t *out_n_present, int32_t *out_n_missing);
int         sh_job_submit_calls_select(sh_job *job, sh_select *sel, const uint8_t *present, const uint8_t *missing, int64_t src_row_bytes, int64_t V,
                                       const int32_t *skip, const char *names, const int64_t *name_off, double max_missing);
/* n_present and n_missing of every row of the call block last collected (those k_calls_select made, for sh_job_submit_calls_select: what the
 * caller's "No observations of ..." lines are said from).  Valid until the next submit. */
int         sh_job_calls_counts(sh_job *job, int64_t *V, const int32_t **n_present, const int32_t **n_missing);

#ifdef __cplusplus
}
#endif
#endif
