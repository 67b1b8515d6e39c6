/*
 * pcoa.h -- C ABI of the MI355X-native PCoA engine (libpcoa_hip.so).
 *
 * Drop-in boundary for ONE path of googlegenomics/spark-examples: VariantsPcaDriver's
 *   getSimilarityMatrix -> computePca
 * (reference: src/main/scala/com/google/cloud/genomics/spark/examples/VariantsPca.scala, below
 * "VariantsPca.scala"; Python twin src/main/python/variants_pca.py, below "variants_pca.py").
 * The reference has no FFI; the seam is the method boundary of class VariantsPcaDriver
 * (VariantsPca.scala:81).  Every entry point below names the reference interface it replaces.
 * The JNI / ctypes bindings a maintainer would add are shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; little-endian int32_t / int64_t / float / double;
 *   - every function returns 0 on success or a negative pcoa_status; it never throws or aborts;
 *     the message of the last failure is available from pcoa_last_error();
 *   - a pcoa_ctx owns all of its device memory and one HIP stream on ONE GPU; the caller owns every
 *     host buffer passed in; a ctx is used from one host thread at a time, different ctxs are
 *     independent (one per Spark task / per rank);
 *   - matrices are row-major unless stated; "device pointer" means HIP device memory on the ctx's GPU;
 *   - accumulate calls only queue work (on the ctx stream and, for device tiles -- fp32, uint8, bitsets --, on two side
 *     streams the ctx owns and orders against it: the pre-pass of one operand buffer runs while the previous one is contracted); the SYNCHRONISING calls are pcoa_sync, pcoa_gram_finalize, every read / load / export /
 *     import / all-reduce / compute call, pcoa_get_timings / pcoa_reset_timings and pcoa_set_stream.  A DEVICE input of an
 *     accumulate call must stay valid and unchanged until the next synchronising call returns: its pre-pass may still be
 *     running, and in the default (auto) mode a tile whose pre-pass met a carrier multiplicity is read a second time by
 *     the int8 path.  HOST inputs are consumed before the accumulate call returns.
 */
#ifndef PCOA_H_
#define PCOA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCOA_VERSION_MAJOR 0
#define PCOA_VERSION_MINOR 19

typedef struct pcoa_ctx pcoa_ctx;

typedef enum pcoa_status {
  PCOA_OK = 0,
  PCOA_ERR_INVALID_ARG = -1,   /* null pointer, negative size, num_pc out of (0, N] ...          */
  PCOA_ERR_NO_DEVICE = -2,     /* no HIP device / ordinal out of range: the product has NO CPU fallback */
  PCOA_ERR_HIP = -3,           /* a HIP runtime call or kernel failed (message has the HIP error) */
  PCOA_ERR_OUT_OF_MEMORY = -4,
  PCOA_ERR_INDEX_RANGE = -5,   /* a callset index outside [0, N): the reference throws here
                                  (mapping(call.callsetId), VariantsPca.scala:59; Breeze bounds check :188) */
  PCOA_ERR_RCCL = -6,
  PCOA_ERR_NOT_CONVERGED = -7, /* no verified eigenpair (Lanczos-only mode, or N too large for the dense fallback) */
  PCOA_ERR_STATE = -8          /* the call does not apply to this kind of ctx (e.g. pcoa_compute on a strip owner) */
} pcoa_status;

/* flags for pcoa_create */
#define PCOA_FLAG_DEFAULT        0u     /* auto: MX-FP4 MFMA for binary (0/1) tiles, int8 MFMA for tiles that
                                           hold carrier multiplicities 2..127 (decided per operand-buffer
                                           generation, both exact; int32 launches and int64 folds are sized by the
                                           largest multiplicity met, so counts never wrap)                      */
#define PCOA_FLAG_GRAM_F32_MFMA  0x1u  /* fp32-MFMA Gram kernel (v_mfma_f32_32x32x2_f32): any small ints */
#define PCOA_FLAG_GRAM_I8_MFMA   0x2u  /* int8-MFMA Gram kernel only (v_mfma_i32_32x32x32_i8), values 0..127 */
#define PCOA_FLAG_GRAM_FP4_MFMA  0x4u  /* MX-FP4 Gram kernel only (v_mfma_f32_32x32x64_f8f6f4): a value
                                           other than 0 / 1 is an error                                        */
#define PCOA_FLAG_NO_SIGN_NORM   0x10u /* keep the eigensolver's native sign instead of sign-normalising */
#define PCOA_FLAG_EIG_HOUSEHOLDER 0x20u /* always use the dense Householder + bisection eigensolver        */
#define PCOA_FLAG_EIG_LANCZOS    0x40u /* Lanczos only: PCOA_ERR_NOT_CONVERGED instead of falling back      */
#define PCOA_FLAG_EIG_BAND       0x200u /* Lanczos as the BAND iteration from the start (block width num_pc + 2) instead of the
                                           single-vector one.  The default runs the single vector first (0.5 ms at N = 2504) and
                                           the band iteration only when that does not verify: clusters of eigenvalues down to a
                                           relative ~1e-12 are resolved either way, but an eigenvalue of EXACT multiplicity m > 1
                                           (a cohort with an exact symmetry: duplicated samples, mirrored populations) shows a
                                           single start vector one direction of its eigenspace only -- the pair that comes back
                                           is verified, yet a twin of the same eigenvalue can be missing from the top num_pc.
                                           This flag finds multiplicities up to num_pc + 2 (~3 ms instead of 0.5 at N = 2504). */
#define PCOA_FLAG_NO_PIPELINE    0x80u /* device tiles: pre-pass and contraction strictly one after the other on the ctx
                                           stream (the default runs the pre-pass of one fp32 / uint8 operand buffer beside
                                           the contraction of the previous one, on two side streams, for N = 1,025 .. 16,384;
                                           bitset tiles, whose pre-pass is a fifth of their contraction, run in series).
                                           The side streams want hardware queues of their own: HIP maps a process's streams
                                           onto a handful of queues per device, so with SEVERAL ctxs alive on ONE device the
                                           two kernels of a ctx can end up back to back (measured: uint8 tiles 1.62 instead of
                                           1.16 ms per step with a second, idle ctx alive) -- one ctx per device is the fast
                                           configuration */
#define PCOA_FLAG_OPERAND_FP4    0x100u /* binary tiles: keep the re-laid-out operand in HBM as MX-FP4 (4 bits per genotype,
                                           the r01 / r02 form) instead of the default k-bits form (1 bit per genotype,
                                           expanded to MX-FP4 in registers by the contraction).  Same MFMA, same S. */

/* Per-stage timings, filled by pcoa_get_timings(); times in seconds, measured with HIP events on
 * the ctx stream.  Counters are cumulative since pcoa_create / pcoa_reset_timings. */
typedef struct pcoa_timings {
  double gram_kernel_seconds;   /* sum of Gram-kernel launch durations                               */
  int64_t gram_kernel_launches;
  int64_t gram_variants;        /* variants pushed through the Gram kernels                           */
  double gram_flops;            /* algorithmic 2*V*N^2                                                */
  double gram_bytes;            /* algorithmic 4*V*N (X read once) + 4*N^2 per launch                 */
  double densify_seconds;       /* CSR -> dense tile kernels                                          */
  double synth_seconds;         /* synthetic genotype generation                                      */
  double finalize_seconds;      /* symmetrise + fold                                                  */
  double center_seconds;        /* row sums + double centring                                         */
  double tridiag_seconds;       /* Householder tridiagonalisation                                     */
  double eig_seconds;           /* tridiagonal eigenvalues + inverse iteration                        */
  double backtransform_seconds; /* reflector back-transform + normalisation                           */
  double compute_total_seconds; /* wall of the last pcoa_compute (centring..D2H)                      */
  int32_t gram_kernel_kind;     /* of the last launch: 1 = fp32 MFMA, 2 = int8 MFMA, 3 = MX-FP4 MFMA */
  int32_t operand_bits;         /* bits per genotype of that launch's operand in HBM: 32 (fp32 tile read in place), 8 (int8),
                                   4 (MX-FP4 operand), 1 (k-bits operand: expanded to MX-FP4 inside the contraction) */
  double pack_seconds;          /* fp32 -> k-blocked int8 pre-pass of the i8 path (sum of launches)   */
  int64_t pack_launches;
  double pack_bytes;            /* algorithmic bytes of the pre-pass: 4*V*N read + V*Npad written     */
  double lanczos_seconds;       /* Lanczos fast path of the eigensolver (sum over computes)           */
  int32_t eig_method;           /* of the last pcoa_compute: 1 = Lanczos (verified), 2 = Householder  */
  int32_t lanczos_steps;        /* Krylov dimension reached by the last pcoa_compute                  */
  int64_t fp4_fallbacks;        /* chunks the auto mode re-ran on the int8 kernel (non-binary values) */
  int64_t lockstep_launches;    /* contraction launches in the lock-step form (all tiles of a k-stream resident)  */
  int64_t pipeline_launches;    /* of those: launched on the contraction stream beside the next buffer's pre-pass
                                   (fp32 pipeline, DESIGN_HISTORY.md 4.1)                                                  */
  int32_t pipeline_pre_pass_cus;    /* CUs the pre-pass runs on while such a contraction does (0 = pipeline unavailable).  k-bits
                                       operand: all of them -- the ring pre-pass SHARES every CU with the contraction --, so
                                       pipeline_pre_pass_cus + pipeline_contraction_cus > the CU count means "co-resident" */
  int32_t pipeline_contraction_cus; /* CUs that contraction occupies (one workgroup each)                        */
  int64_t evensplit_launches;   /* contraction launches in the even-split form (k-bits operand: every workgroup an equal
                                   run of (tile, stage) units, one workgroup per CU)                                */
  /* ---- r04 (read them with pcoa_get_timings_sized; pcoa_get_timings stops in front of them) ---- */
  double csr_stage_seconds;     /* carrier lists: HOST seconds spent copying pageable arrays into pinned staging  */
  double csr_wait_seconds;      /* carrier lists: HOST seconds spent waiting for the device's check of a call     */
  int64_t csr_fast_chunks;      /* chunks (<= 8 M entries) scattered by the device-validated path                */
  int64_t csr_redo_chunks;      /* of those: redone on the int8 kernel because a list repeated a callset           */
  /* ---- r06 ---- */
  double allreduce_seconds;     /* pcoa_gram_allreduce_rccl: HIP-event time of the collective(s) on the ctx stream (agreement
                                   words + the S all-reduce), summed over calls                                            */
  int64_t allreduce_calls;
  int32_t comm_ranks;           /* ncclCommCount of the communicator of the last pcoa_gram_allreduce_rccl (0 = never called) */
  int32_t allreduce_int32;      /* 1 = that call reduced the int32 partial in place (4 N^2 bytes), 0 = the int64 branch     */
  int32_t matvec_form;          /* of the last pcoa_compute's Lanczos: 0 = one wave per row over all N^2 entries, 1 = upper-
                                   triangular tiles (N >= 16,384, no int64 part), 2 = materialised B                        */
  int32_t gram_i64_live;        /* 1 = S currently has an int64 part (counts beyond int32), 0 = S lives in the int32 matrix  */
  int64_t reduce_int32_calls;   /* pcoa_gram_reduce_from calls that took the int32 path (peer copy of 4 N^2 bytes)           */
  int64_t narrowed_to_int32;    /* times an int64 S handed in (import / load / int64 reductions) was found to fit int32 and
                                   moved back into the int32 matrix, which keeps the large-N upper-triangle forms available  */
  int32_t lanczos_block_steps;  /* band-Lanczos fallback (clustered leading eigenvalues): columns (= mat-vecs) it processed in
                                   the last pcoa_compute / pcoa_lanczos_with_matvec, thick restarts included; 0 = the
                                   single-vector iteration sufficed                                                          */
  int32_t eig_dense_form;       /* launch forms the last pcoa_compute's dense solve of the N x N matrix B took, a bit set chosen
                                   by the launchers: 1 fused Householder step (8 <= N <= 6,784), 2 that step
                                   with more than 64 KiB of dynamic LDS (N >= 2,731), 4 two-kernel step (2 <= N <= 7,
                                   N >= 6,785), 8 bisection from LDS (N <= 4,080), 16 inverse iteration from LDS
                                   (N <= 3,490), 32 inverse iteration with one workgroup per vector, 64 blocked compact-WY
                                   back-transform (N >= 130).  0 when eig_method != 2                                        */
  /* ---- 0.7: the implicit similarity operator (pcoa_create_operator) ---- */
  int64_t operator_products;      /* products y = S v / y = B v applied since pcoa_create_operator / pcoa_reset_timings       */
  double operator_matvec_seconds; /* HIP-event time of those products (both passes, the combine stages, the centring terms)   */
  int64_t operator_store_bytes;   /* HBM the bit store holds now (whole segments); 0 on every other kind of ctx               */
  /* ---- 0.8: S of a sample subset (pcoa_create_subset); counted on the ctx that call returned ---- */
  double subset_seconds;          /* HIP-event time of the gathers that filled this ctx's S                                   */
  int64_t subset_bytes;           /* bytes those gathers read and wrote: 8 m^2 for the int32 matrix, 16 m^2 more for an int64
                                     part                                                                                     */
} pcoa_timings;
#define PCOA_TIMINGS_R03_BYTES 192  /* offsetof(pcoa_timings, csr_stage_seconds): what pcoa_get_timings writes */

/* Synthetic genotype model (bench / tests only; not part of the reference).  Sample i belongs to
 * population p iff pop_offsets[p] <= i < pop_offsets[p+1].  Genotype X[v,i] = 1 iff
 * philox4x32-10(key = (seed_lo, seed_hi), counter = (v_lo, v_hi, i/4, 0))[i%4] < thresholds[v*n_pops + p].
 * Pure integer arithmetic => bit-identical on host and device and invariant to sharding. */
typedef struct pcoa_synth_params {
  uint64_t seed;
  int32_t n_pops;
  int32_t reserved;
  const int32_t* pop_offsets;   /* host, n_pops + 1 entries, pop_offsets[n_pops] == n_samples        */
  const uint32_t* thresholds;   /* host, [n_variants][n_pops] for the range being generated          */
} pcoa_synth_params;

/* ---- lifetime ------------------------------------------------------------------------------- */

/* Creates an engine for an N x N similarity matrix on GPU `device_ordinal`.
 * Replaces: the per-partition DenseMatrix.zeros[Int](size, size) (VariantsPca.scala:183-185) plus
 * the SparkContext the driver holds (VariantsPca.scala:83-85).  N = common.indexes.size. */
int pcoa_create(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags);

/* Strip owner (a cohort whose N x N matrix does not fit one HBM -- BASELINE configs[4], 250,000 samples,
 * S = 250 GB).  The ctx holds S[:, col0 .. col0 + cols) only -- every row, the strip's columns, BOTH triangles -- as a
 * row-major [N][cols] matrix; the strips of all owners tile S.  Every owner is fed ALL variants (the accumulate calls
 * below, unchanged; bitsets are 31 KB per variant at N = 250,000), so nothing is all-reduced: the exchange step is the
 * all-gather of an N-vector per Lanczos step (pcoa_strip_matvec).  pcoa_gram_read_i64 / _load_i64 / _export / _import
 * move [N][cols] matrices on a strip ctx, pcoa_gram_read_block_i64 takes (row, strip-relative column).
 * pcoa_center_read_f64 / pcoa_compute / pcoa_gram_allreduce_rccl are not available on it (PCOA_ERR_STATE).
 * Any n_samples >= 1 will do (the smallest owner is n_samples = 1 with the strip (0, 1)); PCOA_ERR_INVALID_ARG for a strip
 * that is empty or does not lie inside [0, n_samples), and for PCOA_FLAG_GRAM_F32_MFMA.
 * Replaces: the same per-partition matrix of getSimilarityMatrix (VariantsPca.scala:183-189), column-sliced; the
 * reference itself stops at N^2 < 2^31 (DenseMatrix[Int]). */
int pcoa_create_strip(pcoa_ctx** out, int32_t n_samples, int32_t col0, int32_t cols, int32_t device_ordinal,
                      uint32_t flags);

/* computePca's eigensolver for a matrix the engine does not hold (r04): the engine's Lanczos iteration (Krylov basis and
 * re-orthogonalisation on the GPU, Ritz pairs by bisection + inverse iteration, a pair accepted only after its TRUE residual
 * passes) with the product y = B v supplied by the caller: fn(user, v_dev, y_dev) must leave B v in y_dev -- both are device
 * vectors of N doubles on the ctx's GPU -- with its own work complete when it returns, and return 0.  out_components:
 * [num_pc][N] unit, sign-normalised columns (as pcoa_compute); PCOA_ERR_NOT_CONVERGED if no verified pair is reached (there
 * is no dense fallback here).  Any ctx will do (a strip owner's: spark-examples_amd/strips.py runs computePca over strips
 * through this, every product one all-gather of an N-vector).  Replaces: the same MLlib call (VariantsPca.scala:224-227). */
typedef int (*pcoa_matvec_fn)(void* user, const double* v_dev, double* y_dev);
int pcoa_lanczos_with_matvec(pcoa_ctx* ctx, int32_t num_pc, pcoa_matvec_fn fn, void* user, double* out_components,
                             double* out_eigenvalues, int32_t* steps_out);

/* Returns 1 for a strip owner (and its column range), 0 for an ordinary ctx. */
int pcoa_strip_info(const pcoa_ctx* ctx, int32_t* col0_out, int32_t* cols_out);

/* out_cols[jj] = sum_i S(i, col0 + jj): the row sum of sample col0 + jj (S is symmetric), an exact integer.
 * Replaces: rowSums (VariantsPca.scala:206) for the strip's samples; the owners' vectors concatenate to rowSums. */
int pcoa_strip_col_sums(pcoa_ctx* ctx, double* out_cols);

/* y_out[jj] = sum_i B(col0 + jj, i) * v[i] with B(j, i) = ((S(j, i) - means[j]) - means[i]) + matrix_mean -- rows of the
 * double-centred matrix in the reference's operation order (VariantsPca.scala:216-221), evaluated on the fly from the
 * strip (B is never stored).  v, means (= rowSums / N, all N samples) and y_out are host arrays.  One call per owner and
 * Lanczos step; the owners' results concatenate (all-gather) to B v.  Every operation is an IEEE fp64 one rounded on its own
 * (no fused multiply-add); the terms of rows i in [256 b, 256 b + 256) are added in order into a partial that starts at 0.0
 * and the partials in order of b into y_out[jj]: deterministic, and a column's result does not depend on the strip's cut. */
int pcoa_strip_matvec(pcoa_ctx* ctx, const double* v, const double* means, double matrix_mean, double* y_out);

/* The same mat-vec for a host whose vectors already live on the GPU (e.g. torch tensors exchanged with an RCCL all-gather):
 * pcoa_strip_set_centering uploads means (host, N doubles) and matrix_mean ONCE per computePca -- they stay resident until
 * S changes -- and pcoa_strip_matvec_device takes v (N doubles) and y (cols doubles) as DEVICE pointers on the ctx's GPU.
 * It returns when y is complete; v must be complete when it is called (synchronise the producing stream first).
 * Nothing crosses PCIe per Lanczos step. */
int pcoa_strip_set_centering(pcoa_ctx* ctx, const double* means, double matrix_mean);
int pcoa_strip_matvec_device(pcoa_ctx* ctx, const double* v_dev, double* y_dev);

/* ---- the implicit similarity operator: principal coordinates without forming S ---------------------------------------
 * With X the V x N carrier bit matrix (row v = the bitset of variant v, what pcoa_accumulate_bits and
 * pcoa_accumulate_plink_bed bring to the device), S = X^T X and S v = X^T (X v): two passes over a 1-bit operand of V N / 8
 * bytes instead of N^2 V matrix-core work and 4 N^2 bytes of S.  computePca's Lanczos iteration touches S only through such
 * products, and the row sums its centring needs are S 1 = X^T (X 1), exact integers.
 *
 * pcoa_create_operator: a ctx that holds the carrier bitsets of every variant it has been fed and NO N x N matrix of any kind;
 * its HBM use is the bit store, the Lanczos workspace, O(N) + O(V) vectors and the partial sums of the two passes
 * (ceil(N / 8192) V + ceil(V / 512) N doubles), so the sample count of one GPU is bounded by "the bitsets fit", not by "S fits".
 *   input:  pcoa_accumulate_bits (host or device pointer) and pcoa_accumulate_plink_bed (host, device, PCOA_BED_HOST_ASYNC;
 *           the same lifetime rules) append to the store.  The dense fp32 / uint8 tiles, the carrier lists (a list can repeat a
 *           callset, a bitset cannot) and pcoa_accumulate_synthetic (it writes the contraction operand, not variant-major
 *           bitsets) return PCOA_ERR_STATE.
 *   store:  segments of a fixed number of rows (about 256 MiB each; whole multiples of 2,048 rows where a segment holds that
 *           many), allocated as the store grows and never reallocated or copied; rows at a fixed pitch of ceil(N / 32) words
 *           rounded up to 4; bits of samples >= N are cleared on append.  An append that cannot get its segments leaves the
 *           store as it was and returns PCOA_ERR_OUT_OF_MEMORY.  pcoa_reset empties the store.
 *   pcoa_compute: the outputs of a full engine ([num_pc][N] unit sign-normalised columns, eigenvalues, non-zero rows): row
 *           sums -> means, matrix mean, non-zero rows -> the Lanczos iteration with the centred product; PCOA_ERR_NOT_CONVERGED
 *           if no verified pair is reached (no dense fallback: there is no matrix).  PCOA_FLAG_EIG_BAND is honoured;
 *           PCOA_FLAG_EIG_HOUSEHOLDER with N >= 32 and the PCOA_FLAG_GRAM_* / PCOA_FLAG_OPERAND_FP4 flags are
 *           PCOA_ERR_INVALID_ARG at create.  N < 32 (below the Lanczos path): the resident segments are fed, as device
 *           bitsets, to a temporary full engine on the same device and its pcoa_compute is returned.
 *   not available (PCOA_ERR_STATE, the ctx stays usable): everything that reads or moves S -- pcoa_gram_read_i64 /
 *           _read_block_i64 / _load_i64 / _export_device_i64 / _import_device_i64, pcoa_gram_reduce_from (either side),
 *           pcoa_gram_allreduce_rccl, pcoa_center_read_f64, pcoa_project (either side), pcoa_compute_strips, the pcoa_strip_*
 *           calls.  pcoa_gram_finalize and pcoa_sync drain the appends; pcoa_reserve reserves the Lanczos workspace and the
 *           first segment.
 *   results are reproducible: the same store and the same v give bit-identical y, run to run and whatever the sizes of the
 *           accumulate calls that filled the store were (no floating-point atomics; the order of every addition is fixed by N,
 *           the segment size and a row's index in the store).
 * Replaces: getSimilarityMatrix's per-partition matrix and its reduceByKey (VariantsPca.scala:183-190) by the rows they are
 * built from (getCallsRdd, :153-168), and computePca (:198-231) over them. */
int pcoa_create_operator(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags);

/* Returns 1 for an operator ctx, 0 otherwise (like pcoa_strip_info).  *variants_out: rows in the store; *store_bytes_out:
 * the HBM its segments hold (whole segments).  Either pointer may be NULL. */
int pcoa_operator_info(const pcoa_ctx* ctx, int64_t* variants_out, int64_t* store_bytes_out);

/* out_n[i] = sum_j S(i, j), exact: one integer pass for the per-variant carrier counts c_v, one for
 * r_i = sum_v bit(v, i) c_v in int64.  Replaces: rowSums (VariantsPca.scala:206). */
int pcoa_operator_row_sums(pcoa_ctx* ctx, int64_t* out_n);

/* One product on DEVICE vectors of N doubles on the ctx's GPU.  centred = 0: y = S v.  centred = 1: y = B v with
 * B(j, i) = ((S(j, i) - m_j) - m_i) + mm (VariantsPca.scala:216-221), applied around the product as
 * y = S v - m (1^T v) - 1 (m^T v) + mm (1^T v) 1; m = rowSums / N and mm come from the exact row sums, computed once and
 * resident until the store changes.  Returns when y is complete (synchronous on the ctx stream, like
 * pcoa_strip_matvec_device); v must be complete when it is called.  Public so that variant-sharded operator engines can be
 * combined by one all-reduce of an N-vector per product.  Replaces: the products inside MLlib's computePrincipalComponents
 * (VariantsPca.scala:224-227). */
int pcoa_operator_matvec_device(pcoa_ctx* ctx, const double* v_dev, double* y_dev, int centred);

/* ---- standardised-genotype PCA (the genetic relationship matrix) as an implicit operator -----------------------------------
 * The PCA of smartpca, plink --pca, GCTA and flashpca decomposes K = Z^T Z / M over allele-frequency-standardised dosages,
 * missing calls mean-imputed -- not the carrier-sharing counts S every other engine here holds.  With the store's V rows of N
 * genotypes, for sample i at variant v:
 *   c_iv in {0, 1}     1 when the sample is called (its .bed code is not 01)
 *   g_iv in {0, 1, 2}  copies of the non-reference allele, chosen by ref_is_a1 as pcoa_accumulate_plink_bed documents; 0 where
 *                      the sample is not called
 * per variant, exact int32:  n_v = sum_i c_iv,  h_v heterozygous samples,  o_v homozygous non-reference samples,  a_v = h_v + 2 o_v
 * per variant, fp64, in exactly these expressions:
 *   mu_v   = a_v / n_v
 *   used_v = n_v > 0 and 0 < a_v < 2 n_v and min(a_v, 2 n_v - a_v) >= min_maf * (2.0 * n_v)
 *   d_v    = used_v ? 1.0 / (mu_v * (1.0 - 0.5 * mu_v)) : 0.0
 *   M'     = sum_v used_v
 * and A_vi = g_iv - mu_v c_iv,  K = A^T diag(d) A / M'.  There is no double centring: every row of A has mean 0 over its called
 * samples.  d_v is applied once, between the two passes of a product, not as a square root in both.
 *
 * pcoa_create_grm: a ctx that holds 2 bits per genotype of every variant it has been fed (626 MB at 2,504 x 10^6) and NO N x N
 * matrix; n_samples < 32 is PCOA_ERR_INVALID_ARG (computePca is the Lanczos iteration), and so are the flags
 * pcoa_create_operator refuses.
 *   input:  pcoa_accumulate_plink_bed only (host, device, PCOA_BED_HOST_ASYNC; the same lifetime rules).  Padding bits of a
 *           row and bytes beyond ceil(N / 4) are ignored.  Every other accumulate call returns PCOA_ERR_STATE.
 *   store:  as an operator ctx's: segments of about 256 MiB, allocated as the store grows and never reallocated or copied; rows
 *           at a pitch of ceil(N / 4) bytes rounded up to 16, in one coding whatever ref_is_a1 was; an append that cannot get
 *           its segments leaves the store as it was (PCOA_ERR_OUT_OF_MEMORY).  pcoa_reset empties the store and keeps min_maf.
 *   pcoa_compute: the outputs of a full engine ([num_pc][N] unit sign-normalised columns, eigenvalues of K) by the Lanczos
 *           iteration over the product; *out_nonzero_rows = the samples called at one or more used variants;
 *           PCOA_FLAG_EIG_BAND is honoured; M' = 0 is PCOA_ERR_STATE; PCOA_ERR_NOT_CONVERGED if no verified pair is reached
 *           (no dense fallback: there is no matrix).
 *   pcoa_reserve, pcoa_sync, pcoa_gram_finalize, pcoa_destroy: as on an operator ctx.  Products count under
 *           operator_products / operator_matvec_seconds of pcoa_timings.
 *   not available (PCOA_ERR_STATE, the ctx stays usable): everything that reads or moves S, and the pcoa_operator_*, strip,
 *           project, subset, pairs, king, similarity, companion, loadings and LD calls.
 *   results are reproducible: the same store, min_maf and x give bit-identical y, run to run and whatever the sizes of the
 *           accumulate calls were (no floating-point atomics; the order of every addition is fixed by N, the segment size
 *           and a row's index in the store).
 * SNP weights and the projection of new samples: pcoa_grm_weights / pcoa_grm_project below.  Reading K out: pcoa_grm_block.
 * LD pruning: pcoa_grm_ld_prune below prunes the RESIDENT store by the r^2 of the dosages and installs a keep mask that enters
 * used_v (so d_v and M' too): the product, pcoa_compute, pcoa_grm_weights, pcoa_grm_project, pcoa_grm_block and the
 * called-sample count see the pruned store; no row is fed twice and none moves.
 * Variant and sample QC: pcoa_grm_set_variant_filters below adds the missing-share and the Hardy-Weinberg conjunct to used_v
 * (off by default); pcoa_grm_hwe and pcoa_grm_sample_counts read the statistics out.
 * Not built: JNI / Scala natives, variant sharding over engines. */
int pcoa_create_grm(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags);

/* Returns 1 for a GRM ctx, 0 otherwise (like pcoa_operator_info).  *variants_out: rows in the store; *used_out: M' under the
 * current min_maf (computes the counts and weights if they are not resident); *store_bytes_out: the HBM the segments hold.
 * Any pointer may be NULL. */
int pcoa_grm_info(pcoa_ctx* ctx, int64_t* variants_out, int64_t* used_out, int64_t* store_bytes_out);

/* 0 <= maf < 0.5 (default 0): a variant is used only if its minor-allele count is at least maf * 2 n_v.  A property of the ctx:
 * it survives pcoa_reset. */
int pcoa_grm_set_min_maf(pcoa_ctx* ctx, double maf);

/* out[(v - first_variant) * 3 + {0, 1, 2}] = n_v, h_v, o_v (called, heterozygous, homozygous non-reference) of the store's rows
 * [first_variant, first_variant + n_variants); host memory. */
int pcoa_grm_counts(pcoa_ctx* ctx, int64_t first_variant, int64_t n_variants, int32_t* out /* [n_variants][3] */);

/* y = K x on DEVICE vectors of N doubles on the ctx's GPU; returns when y is complete (synchronous on the ctx stream), x must
 * be complete when it is called.  M' = 0 gives y = 0. */
int pcoa_grm_matvec_device(pcoa_ctx* ctx, const double* x_dev, double* y_dev);

/* ---- SNP weights of the axes of K, and new samples projected onto them -------------------------------------
 * With K u_c = lambda_c u_c (what pcoa_compute returned on the panel) and Z = D^1/2 A / sqrt(M'):
 *   t_vc = d_v (A u_c)_v                                  the first pass of the product applied to u_c
 *   w_vc = sqrt(d_v) (A u_c)_v / sqrt(M' lambda_c)         the left singular vectors of Z: smartpca's snpweightoutname, plink2's
 *                                                          --pca var-wts (up to their scaling conventions)
 *   u_c[i] = sum_v A_vi t_vc / (M' lambda_c), so a sample q genotyped at the same variants is placed at
 *   coord(q, c) = sum_v (g_vq - mu_v c_vq) t_vc / (M' lambda_c)
 * with mu, d and M' the PANEL's; a missing call of q contributes 0 (mean imputation, as in K itself).  The panel's own samples
 * come back as u_c.  The panel's counts and weights are recomputed, if they are not resident, under its current min_maf, as
 * pcoa_compute does.  Both calls run the passes for two components at a time; every column is added in the order of the
 * one-vector product, so component c has the same bits whatever num_pc is, and a study store that holds the panel's own rows
 * gives pcoa_grm_matvec_device(u_c) / lambda_c bit for bit.  Neither call writes a store, and every error leaves both ctxs
 * usable.  PCOA_ERR_STATE: panel is not a pcoa_create_grm ctx.  PCOA_ERR_INVALID_ARG: num_pc < 1, an eigenvalue that is not
 * positive and finite, M' = 0, a window outside the store, a NULL output.
 *
 * pcoa_create_grm_study: a GRM store of n_samples >= 1 study samples: pcoa_accumulate_plink_bed, pcoa_grm_info (used_out = 0),
 * pcoa_grm_counts, pcoa_reset / reserve / sync / destroy as on a GRM ctx; it has no weights of its own: pcoa_compute,
 * pcoa_grm_matvec_device and pcoa_grm_set_min_maf return PCOA_ERR_STATE with their own message.  Flags as pcoa_create_grm.
 * A sample called at a share f of the used variants lands at about f times its position (out_called lets a host report the
 * shrinkage); pcoa_grm_project_lsq below places it by least squares over the variants it IS called at.
 * Not built: a saved model, allele flipping between the two filesets, multi-GPU, JNI / Scala natives. */
int pcoa_create_grm_study(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags);

/* scaled = 0: out[(v - first_variant) * num_pc + c] = t_vc (the vector the projection uses; 0 for an unused variant)
 * scaled = 1: w_vc = used_v ? t_vc / sqrt(d_v * ((double)M' * lambda_c)) : 0.0   in exactly this expression, no contraction
 * components: host [num_pc][N]; eigenvalues: host [num_pc]; out: host [n_variants][num_pc]. */
int pcoa_grm_weights(pcoa_ctx* panel, int32_t num_pc, const double* components, const double* eigenvalues, int32_t scaled,
                     int64_t first_variant, int64_t n_variants, double* out);

/* out_coords[c * N_study + q] = (sum_v g_vq t_vc + sum_v c_vq s_vc) / M' / lambda_c with s_vc = -(mu_v t_vc), the partial sums
 * added in (segment, range) order of the STUDY's store; out_called[q] (may be NULL) = the panel's USED variants at which q is
 * called.  study: either GRM kind (the panel itself included), on the panel's device (PCOA_ERR_INVALID_ARG otherwise), holding
 * exactly as many rows as the panel, fed in the same order (PCOA_ERR_STATE otherwise). */
int pcoa_grm_project(pcoa_ctx* panel, pcoa_ctx* study, int32_t num_pc, const double* components, const double* eigenvalues,
                     double* out_coords /* [num_pc][N_study] */, int32_t* out_called /* [N_study] */);

/* ---- least-squares projection of sparsely called samples ----------------------------------------------------
 * smartpca's lsqproject.  With the unit weights w_vc = t_vc / sqrt(d_v M' lambda_c) and z_vq = sqrt(d_v) (g_vq - mu_v) / sqrt(M'),
 * the coordinates of study sample q minimise sum over the used variants q is CALLED at of (z_vq - sum_c w_vc sqrt(lambda_c) x_c)^2.
 * M' and sqrt(lambda) cancel from the normal equations, so the call takes no eigenvalues.  With K = num_pc, per sample q:
 *   P_q[c]    = sum_v (g_vq - mu_v c_vq) * t_vc                 the numerator pcoa_grm_project forms: P_q[c] / M' / lambda_c has
 *                                                               the bits of its output
 *   p_v[c,c'] = used_v ? (t_vc * t_vc') / d_v : 0.0             in exactly this expression, no contraction;  c' <= c
 *   H_q[c,c'] = sum_v c_vq * p_v[c,c']                          K (K + 1) / 2 sums; the rows of a range of 512 in order, the ranges
 *                                                               in (segment, range) order of the STUDY's store, like P
 *   x_q       = the solution of H_q x = P_q
 * For a fully called sample and true eigenvectors H_q = diag(M' lambda_c) and x_q is pcoa_grm_project's coordinate.  A pair's sum
 * has the same bits whatever num_pc is.  The solve is a Cholesky factorisation without pivoting in its square-root-free form
 * H = L D L^T (so that num_pc = 1 gives x = P / H bit for bit), components in the order c = 0 .. K - 1, in fp64 with every product
 * and difference rounded on its own (no contraction), in exactly this sequence (h = H_q packed, h[c][j] at c (c + 1) / 2 + j):
 *   for c = 0 .. K-1:   hcc = h[c][c];                                    undetermined if hcc == 0
 *     for j = 0 .. c-1: s = h[c][j];  for k = 0 .. j-1: s = s - h[c][k] * h[j][k];   h[c][j] = s          (s = L[c][j] D[j])
 *     s = hcc;  for k = 0 .. c-1: w = h[c][k];  l = w / h[k][k];  s = s - w * l;  h[c][k] = l            (l = L[c][k])
 *     pivot_c = s;                                                        undetermined if pivot_c <= 2^-40 * hcc
 *     h[c][c] = pivot_c                                                                                   (D[c])
 *   for c = 0 .. K-1:   s = P[c];  for k = 0 .. c-1: s = s - h[c][k] * y[k];   y[c] = s
 *   for c = 0 .. K-1:   z[c] = y[c] / h[c][c]
 *   for c = K-1 .. 0:   s = z[c];  for k = c+1 .. K-1: s = s - h[k][c] * x[k];   x[c] = s
 * An undetermined sample -- one called at fewer than K used variants always is -- gets NaN in all K coordinates and
 * out_determined[q] = 0; the factorisation stops at the first failing test.
 * out_coords[c * N_study + q]; out_called as pcoa_grm_project; out_normal (may be NULL): [K (K + 1) / 2 + K][N_study], H_q packed
 * (entry c (c + 1) / 2 + c') and then P_q, as they were before the solve.  1 <= num_pc <= 16 (136 pair sums).  Preconditions and
 * error codes are pcoa_grm_project's: PCOA_ERR_STATE for a panel that is not a pcoa_create_grm ctx, a study that is no GRM ctx or
 * holds another number of rows; PCOA_ERR_INVALID_ARG for another device, num_pc outside [1, 16], M' = 0, NULL components or
 * out_coords.  Every error leaves both ctxs usable, nothing writes either store, and the panel's counts and weights are
 * recomputed, if they are not resident, under its current min_maf, filters and LD mask.  pcoa_grm_project is unchanged.
 * Not built: weights per variant beyond d_v, a ridge term for nearly undetermined samples, more than 16 components, JNI / Scala
 * natives. */
int pcoa_grm_project_lsq(pcoa_ctx* panel, pcoa_ctx* study, int32_t num_pc, const double* components /* host [num_pc][N] */,
                         double* out_coords /* host [num_pc][N_study] */, int32_t* out_called /* [N_study] or NULL */,
                         int32_t* out_determined /* [N_study] 1 / 0, or NULL */,
                         double* out_normal /* [num_pc (num_pc + 1) / 2 + num_pc][N_study] or NULL */);

/* What pcoa_grm_project_lsq did with THIS ctx as the panel, cumulative since pcoa_create_grm / pcoa_reset_timings.  It grows at its
 * end; out_size = sizeof of the struct the caller compiled against.  Synchronising. */
typedef struct pcoa_grm_lsq_stats {
  int64_t grm_lsq_calls;
  int64_t grm_lsq_pair_vectors;     /* product vectors p[c,c'] streamed past the study's store: num_pc (num_pc + 1) / 2 per call */
  double grm_lsq_pairs_seconds;     /* HIP-event time of the product, pair and finish launches                                   */
  double grm_lsq_solve_seconds;     /* HIP-event time of the solve                                                               */
  int64_t grm_lsq_undetermined;     /* undetermined samples of the LAST call                                                     */
} pcoa_grm_lsq_stats;
int pcoa_get_grm_lsq_stats(pcoa_ctx* panel, pcoa_grm_lsq_stats* out, size_t out_size);

/* ---- reading K out in blocks --------------------------------------------------------------------------------
 * GCTA --make-grm, plink --make-grm-bin and smartpca also write the matrix they decompose.  pcoa_grm_block returns any
 * rectangle of it, and of the pair counts, computed from the store on the fp64 matrix cores.  The rule, with c, g, n_v, a_v,
 * mu_v, used_v, d_v and M' exactly as pcoa_create_grm defines them and a_vi = c_iv ? (double)g_iv - mu_v : 0.0:
 *   num(i, j) = sum_v (d_v * a_v,lo) * a_v,hi       lo = min(i, j), hi = max(i, j): d rides on the operand of the smaller
 *                                                   sample index, applied once (not as a square root on both sides)
 *   n(i, j)   = sum_v used_v * c_iv * c_jv          exact integer: the used variants at which both samples are called
 *   PCOA_GRM_DIVISOR_USED      (0)   K(i, j) = num(i, j) / (double)M'                      the K that pcoa_compute decomposes
 *   PCOA_GRM_DIVISOR_PAIRWISE  (1)   K(i, j) = n(i, j) > 0 ? num(i, j) / (double)n(i, j) : 0.0
 * A missing call contributes 0 to num, so num is the sum over the jointly called used variants of
 * (g_i - 2p)(g_j - 2p) / (2p(1 - p)): the PAIRWISE form is the pairwise-complete estimator GCTA-style tools store, the USED form
 * the mean-imputed K above.  The diagonal follows the same expression as every other entry.  This rule is the contract, not
 * any tool's output (tools differ in how they treat missing calls, the diagonal and the frequency estimate).
 *   exact symmetry:   K(i, j) and K(j, i) are the same bits (an entry below the diagonal is computed with the operand roles
 *           exchanged, and the multiplicands of a product commute).
 *   cut independence: the bits of an entry depend only on the store, min_maf, the divisor and (i, j): not on the rectangle it
 *           was requested in, the grid, the CU count or the sizes of the accumulate calls.  No floating-point atomics: the
 *           additions into an entry happen in the order of the variants' indices in the store, four at a time within a segment.
 *   exactness: where every used mu_v = 1 and d_v = 2 every partial sum is a small integer and num is exact.
 * Any rectangle inside [0, N)^2; out_k / out_pairs: [rows][cols] row-major, either may be NULL (not both), host memory or, with
 * is_device_ptr, device memory on the ctx's GPU (both outputs alike).  Synchronising.  The counts and weights are recomputed,
 * if they are not resident, under the current min_maf, as pcoa_compute does.  Nothing writes the store; the ctx computes the
 * same bits afterwards.
 *   PCOA_ERR_INVALID_ARG, found on the host before any device work: ctx NULL (pcoa_last_error(NULL)), rows or cols < 1, a
 *           rectangle that leaves [0, N), an unknown divisor, both outputs NULL.
 *   PCOA_ERR_STATE, the ctx stays usable: a ctx that is not from pcoa_create_grm (the message names its kind), a
 *           pcoa_create_grm_study ctx, M' = 0, M' >= 2^31 (the pair counts are int32).
 *   memory: rows * cols doubles, plus as many int32 where the pair counts are needed (out_pairs given, or PAIRWISE), in one
 *           lazily grown buffer of the ctx; a device output is used directly instead.  PCOA_ERR_OUT_OF_MEMORY leaves the ctx
 *           usable.
 * Not built: fp32 / bf16 approximations, multi-GPU, a compressed writer, JNI / Scala natives. */
#define PCOA_GRM_DIVISOR_USED 0
#define PCOA_GRM_DIVISOR_PAIRWISE 1
int pcoa_grm_block(pcoa_ctx* ctx, int32_t row0, int32_t rows, int32_t col0, int32_t cols, int32_t divisor,
                   double* out_k /* [rows][cols] row-major, or NULL */, int32_t* out_pairs /* [rows][cols] n(i, j), or NULL */,
                   int is_device_ptr /* both outputs: host (0) or device memory on the ctx's GPU (1) */);

/* What pcoa_grm_block did on THIS engine, cumulative since pcoa_create_grm / pcoa_reset_timings.  (A struct of its own, like
 * pcoa_pairs_stats.)  It grows at its end; out_size = sizeof of the struct the caller compiled against.  Synchronising. */
typedef struct pcoa_grm_block_stats {
  double grm_block_seconds;   /* HIP-event time of the segment launches and the finish                                        */
  int64_t grm_block_calls;
  double grm_block_flops;     /* 2 * rows * cols * V per float pass launched (num; n where the pair counts are needed)        */
} pcoa_grm_block_stats;
int pcoa_get_grm_block_stats(pcoa_ctx* ctx, pcoa_grm_block_stats* out, size_t out_size);

/* ---- the relatedness cut-off on K ----------------------------------------------------------------------------
 * gcta --grm-cutoff and plink --rel-cutoff find the pairs of samples whose relationship exceeds a threshold.  pcoa_grm_pairs
 * screens the upper triangle of K on the device, a band of rows at a time, and returns only the pairs: no N x N matrix leaves
 * the device.  The rule, with K(i, j) EXACTLY the bits pcoa_grm_block returns for the same ctx, min_maf, keep mask and divisor:
 *   the pair (i, j), i < j, is REPORTED iff K(i, j) >= cutoff
 * one fp64 comparison on the value already divided (variants_pca.py's grm_pairs_rule is the numpy statement).  Pairs come out
 * in increasing (i, j) order, written in order and not sorted.  Content and order are a function of the store, min_maf, the LD
 * keep mask, the divisor and the cutoff alone: not of band_rows, the grid, the CU count or the sizes of the accumulate calls.
 *   band_rows: rows of K held at a time, a multiple of 64; 0 = 1,024.  The band [r0, r0 + band_rows) x [64 floor(r0 / 64), N) is
 *           computed by pcoa_grm_block's kernels into the ctx's workspace, then counted, scanned and written (csrc/grm_pairs.hip);
 *           one launch chain per band, no host synchronisation between bands.
 *   out_pairs / capacity / *n_found_out: as pcoa_similar_pairs -- the first min(n_found, capacity) pairs, entries behind them
 *           untouched; capacity 0 is the count-only call; *n_found_out is always the full count.
 *   a pair's n: n(i, j) under PCOA_GRM_DIVISOR_PAIRWISE, M' under PCOA_GRM_DIVISOR_USED.
 *   out_diag: N doubles or NULL: K(i, i) under the same divisor (the band holds its diagonal tiles).
 * Synchronising.  Nothing writes the store; the ctx computes the same bits afterwards.
 *   PCOA_ERR_INVALID_ARG, found on the host before any device work: ctx NULL (pcoa_last_error(NULL)), n_found_out NULL, a cutoff
 *           that is not finite, an unknown divisor, band_rows negative or not a multiple of 64, capacity < 0, capacity > 0 with
 *           out_pairs NULL.
 *   PCOA_ERR_STATE, the ctx stays usable: as pcoa_grm_block -- a ctx that is not from pcoa_create_grm, a pcoa_create_grm_study
 *           ctx, M' = 0, M' >= 2^31.
 *   memory: band_rows * 64 ceil(N / 64) doubles, plus as many int32 under PAIRWISE, in the lazily grown buffer pcoa_grm_block
 *           uses; the (row, tile) counts, the row offsets and min(capacity, N (N - 1) / 2) records for the length of the call,
 *           all allocated before the first launch.  PCOA_ERR_OUT_OF_MEMORY leaves the ctx usable.
 * Not built: a threshold fused into the dense product's epilogue, skipping the tiles of a band's first block that lie below
 * the diagonal, multi-GPU, GCTA's own removal order, JNI / Scala natives.  (The KING screen over the 2-bit store is
 * pcoa_grm_king_pairs, below.) */
typedef struct pcoa_grm_pair { int32_t i, j; double k; int64_t n; } pcoa_grm_pair;   /* i < j, k = K(i, j); 24 bytes */
int pcoa_grm_pairs(pcoa_ctx* ctx, double cutoff, int32_t divisor, int32_t band_rows /* 0: 1,024 */, pcoa_grm_pair* out_pairs,
                   int64_t capacity, int64_t* n_found_out, double* out_diag /* N doubles, or NULL */);

/* What pcoa_grm_pairs did on THIS engine, cumulative since pcoa_create_grm / pcoa_reset_timings.  (A struct of its own, like
 * pcoa_pairs_stats.)  It grows at its end; out_size = sizeof of the struct the caller compiled against.  Synchronising. */
typedef struct pcoa_grm_pairs_stats {
  double grm_pairs_seconds;          /* HIP-event time of every launch of the calls: the dense bands and the screen          */
  double grm_pairs_screen_seconds;   /* of which the count, scan and write kernels                                           */
  int64_t grm_pairs_calls;
  int64_t grm_pairs_bands;
  double grm_pairs_flops;            /* 2 * band rows * band columns * V per float pass of the dense part                    */
  int64_t grm_pairs_bytes;           /* bytes of the bands the count and write kernels read                                  */
} pcoa_grm_pairs_stats;
int pcoa_get_grm_pairs_stats(pcoa_ctx* ctx, pcoa_grm_pairs_stats* out, size_t out_size);

/* ---- LD pruning of the resident GRM store by dosage r^2 ------------------------------------------------------
 * smartpca, plink --pca, GCTA and flashpca workflows LD-prune the variants in front of the PCA; the accepted pair statistic
 * (plink --indep-pairwise) is the squared Pearson correlation of the DOSAGES over the samples called at both variants -- not the
 * r^2 of carrier indicators that pcoa_ld_* tests.  The rule, all integers up to the last comparison.  Rows are the store's rows
 * in feed order; g_iv in {0, 1, 2} is the dosage and c_iv the called indicator as the store codes them (00 / 10 / 11: g = 0 /
 * 1 / 2; 01: not called).  For two rows u < v let J be the samples called at both; over i in J, in int64:
 *   n = |J|     s_u = sum g_iu     s_v = sum g_iv     q_u = sum g_iu^2     q_v = sum g_iv^2     p = sum g_iu g_iv
 *   cov = n p - s_u s_v      var_u = n q_u - s_u^2      var_v = n q_v - s_v^2
 *   exceeds(u, v)  <=>  (double)cov * (double)cov  >  t * ((double)var_u * (double)var_v)
 * -- three fp64 products and one comparison, no sum and no contraction.  A pair with n = 0, or with a row that is constant on
 * J, has cov = 0 and never exceeds.  A row is a CANDIDATE iff used_v holds under the ctx's current min_maf (the expression of
 * pcoa_create_grm, judged WITHOUT an installed mask).  The pass is the forward greedy pass of pcoa_ld_*: a non-candidate is
 * removed and blocks nobody; a candidate v is kept iff no KEPT u has exceeds(u, v), where v - window <= u < v and u lies behind
 * the last break at or before v.  window counts store rows, not candidates.
 * This is NOT plink --indep-pairwise to the bit: plink slides a window with a step and removes the lower-MAF member of an
 * exceeding pair; here the earlier kept row wins, as in pcoa_ld_*.  The pair statistic is plink's.
 *
 * pcoa_grm_ld_prune: 1 <= window <= PCOA_LD_MAX_WINDOW, 0 <= r2_max <= 1 (NaN refused); breaks: a host array of n_breaks strictly
 * increasing row indices in (0, V) -- "a break lies in front of row b" -- or NULL with n_breaks = 0.  Computes the counts and
 * weights under the current min_maf if they are not resident, runs the pass over the whole store, installs the mask and marks
 * the weights stale, so that the next consumer sees the pruned used_v, d_v (0 for a removed row; mu_v unchanged) and M' (the
 * kept rows).  Synchronising.  *candidates_out / *kept_out (either may be NULL): the candidates and the kept rows; V = 0 gives 0
 * and 0.  A second call replaces the mask; candidates are always judged without the old one.
 * pcoa_grm_ld_mask: out[v - first_variant] = 1 for a kept row, 0 for a removed one (non-candidates included); host memory;
 * PCOA_ERR_STATE without an installed mask.
 * Lifetime: the mask is a statement about the store as it was pruned.  It is dropped by pcoa_grm_ld_clear, pcoa_reset, any
 * pcoa_accumulate_plink_bed that appends at least one row, and pcoa_grm_set_min_maf with a value other than the current one
 * (the same value keeps it).  After a drop pcoa_grm_info reports the unpruned M' again.
 * Errors, all leaving the ctx, the store and an earlier mask as they were:
 *   PCOA_ERR_STATE        a ctx that is not from pcoa_create_grm (the message names its kind); a pcoa_create_grm_study ctx
 *   PCOA_ERR_INVALID_ARG  the ranges above, a NULL breaks with n_breaks > 0, breaks not increasing or out of range, N >= 2^28
 *                         (the sums of a pair are int32 per entry)
 *   PCOA_ERR_OUT_OF_MEMORY the work buffers: [window + C][pitch] row words, C <= 65,536 rows and <= 256 MiB, C band rows of
 *                         ceil(window / 32) words, and V bytes
 * pcoa_ld_* on a GRM ctx stay PCOA_ERR_STATE.  pcoa_grm_project needs nothing new: the study is placed with the panel's pruned
 * used_v.  Not built: plink's step and MAF-ordered removal, windows in base pairs, JNI / Scala natives. */
int pcoa_grm_ld_prune(pcoa_ctx* ctx, int32_t window, double r2_max, const int64_t* breaks, int64_t n_breaks,
                      int64_t* candidates_out, int64_t* kept_out);
int pcoa_grm_ld_mask(pcoa_ctx* ctx, int64_t first_variant, int64_t n_variants, uint8_t* out /* host */);
int pcoa_grm_ld_clear(pcoa_ctx* ctx);

/* What the LAST pcoa_grm_ld_prune of this engine did, and the HIP-event time of the pass's kernels, cumulative since
 * pcoa_create_grm / pcoa_reset_timings.  (A struct of its own, sized like pcoa_ld_stats: it grows at its end; out_size = sizeof
 * of the struct the caller compiled against.)  Synchronising. */
typedef struct pcoa_grm_ld_stats {
  int64_t grm_ld_variants;        /* rows of the store the pass went over                                                    */
  int64_t grm_ld_candidates;      /* of them candidates (used_v under min_maf)                                               */
  int64_t grm_ld_kept;            /* of them kept                                                                            */
  int64_t grm_ld_pairs;           /* in-window pairs (u, v) behind the breaks, candidates or not: what the band kernel tested */
  double grm_ld_band_seconds;     /* reach + band kernel                                                                     */
  double grm_ld_resolve_seconds;  /* the greedy pass (one wave)                                                              */
  double grm_ld_scan_seconds;     /* keep flags to bytes, counts                                                             */
} pcoa_grm_ld_stats;
int pcoa_get_grm_ld_stats(pcoa_ctx* ctx, pcoa_grm_ld_stats* out, size_t out_size);

/* ---- sample subsets of the resident GRM store -----------------------------------------------------------------
 * smartpca removes outliers in rounds and re-estimates the allele frequencies on the survivors; the usual biobank recipe computes
 * the axes on an unrelated subset and projects the excluded samples.  A GRM ctx keeps 2 bits per genotype and nothing else, so
 * the reduced cohort's engine is the same rows with the removed samples' columns taken out: one gather over the store, no
 * variant is fed twice.
 *
 * pcoa_create_grm_subset creates a NEW GRM ctx over n_keep samples on src's device, with src's create flags and src's min_maf:
 * as from pcoa_create_grm (PCOA_GRM_SUBSET_PANEL, n_keep >= 32) or from pcoa_create_grm_study (PCOA_GRM_SUBSET_STUDY, n_keep >=
 * 1).  Its store holds as many rows as src's, in the same order; slot a of row v is slot keep[a] of src's row v, in the store's
 * one coding at the result's own pitch (ceil(n_keep / 4) bytes rounded up to 16); every slot at index >= n_keep, the pitch's
 * padding included, holds 01, exactly as the append leaves a store.  An engine created with n_keep samples and fed the same rows
 * re-packed on the host with ref_is_a1 = 1 is indistinguishable from it, bit for bit, in every later call: the counts, weights
 * and M' are not resident and are computed lazily from its own columns (n_v, mu_v, used_v, d_v, M' of the kept samples).
 *   keep:   a host array of n_keep strictly increasing indices in [0, N_src), consumed on return (pcoa_create_subset's rules).
 *   src:    either GRM kind, a result of this call included.  It is synchronised and otherwise unchanged: it may be fed further,
 *           subset again or destroyed.  A keep mask installed by pcoa_grm_ld_prune on src is NOT inherited (it is a statement
 *           about src's frequencies).  An empty src store gives an empty result.
 *   memory: src's store plus the result's at the peak; all of the result's segments are allocated before the first row moves.
 *   errors are reported on src (pcoa_last_error(src)); *out = NULL and src stays usable:
 *           PCOA_ERR_INVALID_ARG, found on the host before any device work: out / src / keep NULL, an unknown kind, n_keep below
 *             the kind's minimum, an index outside [0, N_src), indices not strictly increasing
 *           PCOA_ERR_STATE: src is not a GRM ctx (the message names its kind)
 *           PCOA_ERR_OUT_OF_MEMORY: the result's segments
 * pcoa_create_subset, the strip calls and every other stored-S call on a GRM ctx stay PCOA_ERR_STATE.
 *
 * pcoa_grm_rows reads rows [first_variant, first_variant + n_variants) of the store back as .bed rows of ceil(N / 4) bytes, in
 * the store's coding, which is a .bed row with ref_is_a1 = 1 (00 g = 0, 01 missing, 10 g = 1, 11 g = 2); the unused slots of the
 * last byte are 00, PLINK's convention.  Either GRM kind.  Feeding the output to a fresh engine with ref_is_a1 = 1 reproduces the
 * store.  Synchronising; no kernel runs.  PCOA_ERR_INVALID_ARG: a window outside the store, a NULL out.
 * pcoa_grm_king_pairs on the source, then this call on the samples to keep, is the KING screen that feeds a GRM engine in one run.
 * Not built: JNI / Scala natives. */
#define PCOA_GRM_SUBSET_PANEL 0   /* result as from pcoa_create_grm       (n_keep >= 32) */
#define PCOA_GRM_SUBSET_STUDY 1   /* result as from pcoa_create_grm_study (n_keep >= 1)  */
int pcoa_create_grm_subset(pcoa_ctx** out, pcoa_ctx* src, const int32_t* keep, int32_t n_keep, int32_t kind);
int pcoa_grm_rows(pcoa_ctx* ctx, int64_t first_variant, int64_t n_variants, uint8_t* out /* host, [n_variants][ceil(N/4)] */);

/* What pcoa_create_grm_subset did with THIS engine as src, cumulative since its creation / pcoa_reset_timings.  (A struct of its
 * own; it grows at its end; out_size = sizeof of the struct the caller compiled against.)  Synchronising. */
typedef struct pcoa_grm_subset_stats {
  double grm_subset_seconds;   /* HIP-event time of the gather launches                                                      */
  int64_t grm_subset_calls;
  int64_t grm_subset_bytes;    /* rows * (src pitch + result pitch) bytes per call: what an ideal gather reads and writes   */
} pcoa_grm_subset_stats;
int pcoa_get_grm_subset_stats(pcoa_ctx* ctx, pcoa_grm_subset_stats* out, size_t out_size);

/* ---- variant and sample QC on the resident GRM store -----------------------------------------------------------
 * Every smartpca / plink --pca / GCTA recipe starts with four filters: --maf (pcoa_grm_set_min_maf), --geno (variant call rate),
 * --hwe (Hardy-Weinberg exact test) and --mind (sample call rate).  The two variant filters are properties of a GRM ctx like
 * min_maf; the sample filter is a host's use of pcoa_grm_sample_counts and pcoa_create_grm_subset.
 *
 * pcoa_grm_set_variant_filters: 0 <= max_missing <= 1 (default 1 = off), 0 <= hwe_min_p < 1 (default 0 = off).  used_v of
 * pcoa_create_grm gains two conjuncts, in exactly these expressions, N the ctx's sample count:
 *   (double)(N - n_v) <= max_missing * (double)N        plink --geno: removed when the missing share exceeds max_missing
 *   hwe_min_p == 0  or  p_v >= hwe_min_p                plink --hwe:  removed when p_v is below hwe_min_p
 * With the defaults used_v is what it is without them, bit for bit.  Like min_maf the filters survive pcoa_reset, are inherited
 * by pcoa_create_grm_subset (which re-derives counts, p-values and used_v from its own columns), mark the weights stale and drop
 * an installed LD keep mask when a value other than the current one is set (the same values keep it), and are what
 * pcoa_grm_ld_prune judges its candidates under.  Every consumer of used_v sees them: the product, pcoa_compute,
 * pcoa_grm_weights, pcoa_grm_project, pcoa_grm_block, pcoa_grm_pairs and the called-sample count.
 *   PCOA_ERR_STATE        a pcoa_create_grm_study ctx and every ctx that is not from pcoa_create_grm (the message names the kind)
 *   PCOA_ERR_INVALID_ARG  NaN or a value outside its range; hwe_min_p > 0 with N >= 2^26 (the tie rule below needs it)
 *
 * pcoa_grm_hwe: out[v - first_variant] = p_v of the store's rows [first_variant, first_variant + n_variants); host memory; either
 * GRM kind; independent of the filters.  The rule (Wigginton, Cutler and Abecasis 2005, without mid-p: plink --hwe's default):
 * with n = n_v, h = h_v, a = h_v + 2 o_v and R = min(a, 2n - a), for the k of R's parity in [0, R]
 *   P(k) = n! R! (2n - R)! 2^k / ( ((R - k) / 2)! k! (n - (R + k) / 2)! (2n)! )
 *   p_v  = sum of P(k) over the k with P(k) <= P(h) * (1 + 2^-24)
 *   p_v  = 1.0 when n = 0 or R = 0
 * The tolerance keeps exact ties counted.  Evaluated in fp64 by the recurrence outward from the mode with the mode's term taken
 * as 1, no contraction; terms that underflow to 0 are dropped.  The p-values are computed only when hwe_min_p > 0 or
 * pcoa_grm_hwe asks, are resident beside the counts and are dropped with them.
 *
 * pcoa_grm_sample_counts: out[i * 3 + {0, 1, 2}] = the rows at which sample i is called, heterozygous, homozygous non-reference;
 * exact int64; host memory, N * 3 entries.  rows: PCOA_GRM_ROWS_ALL (every row of the store; either GRM kind) or
 * PCOA_GRM_ROWS_USED (the rows with used_v under min_maf, the filters and an installed LD mask; PCOA_ERR_STATE on a study ctx).
 * An empty store gives zeros.  Synchronising.  One launch per segment: a lane keeps one word column of 16 samples and counts
 * the three classes of the rows streaming past it with carry-save adders into bit-sliced counters (csrc/grm_qc.hip).
 * Every error leaves the ctx usable.
 * Not built: plink's inbreeding coefficient F, mid-p, per-population HWE, JNI / Scala natives. */
int pcoa_grm_set_variant_filters(pcoa_ctx* ctx, double max_missing /* [0, 1], default 1 = off */,
                                 double hwe_min_p /* [0, 1), default 0 = off */);
int pcoa_grm_get_variant_filters(const pcoa_ctx* ctx, double* max_missing_out, double* hwe_min_p_out);
int pcoa_grm_hwe(pcoa_ctx* ctx, int64_t first_variant, int64_t n_variants, double* out /* host */);
#define PCOA_GRM_ROWS_ALL  0
#define PCOA_GRM_ROWS_USED 1   /* used_v under min_maf, the filters and an installed LD mask; STATE on a study ctx */
int pcoa_grm_sample_counts(pcoa_ctx* ctx, int32_t rows, int64_t* out /* host, [N][3]: called, het, hom non-reference */);

/* What the QC calls did on THIS engine, cumulative since its creation / pcoa_reset_timings, and the variants of the store that
 * fail each of the three variant tests under the CURRENT settings, each test judged alone (a variant may fail several; 0 on a
 * ctx that is not from pcoa_create_grm): MAF = not (n_v > 0 and 0 < a_v < 2 n_v and the min_maf conjunct), so monomorphic and
 * uncalled variants count there.  Computes the counts, and the p-values where hwe_min_p > 0, if they are not resident.  (A struct
 * of its own; it grows at its end; out_size = sizeof of the struct the caller compiled against.)  Synchronising. */
typedef struct pcoa_grm_qc_stats {
  double grm_qc_hwe_seconds;             /* HIP-event time of the HWE kernel                                                 */
  int64_t grm_qc_hwe_calls;              /* its launches (once per store contents, not per pcoa_grm_hwe)                     */
  double grm_qc_sample_counts_seconds;   /* HIP-event time of the sample-count launches and their finish                     */
  int64_t grm_qc_sample_counts_calls;
  int64_t grm_qc_fail_maf;
  int64_t grm_qc_fail_missing;
  int64_t grm_qc_fail_hwe;
} pcoa_grm_qc_stats;
int pcoa_get_grm_qc_stats(pcoa_ctx* ctx, pcoa_grm_qc_stats* out, size_t out_size);

/* ---- PCoA over a sample subset of a stored S ------------------------------------------------------------------------------
 * For a kept index set I, S[I, I] is exactly the similarity matrix of the reduced cohort (an entry counts the variants two
 * samples share; no other sample enters it), and the centring and the eigenpairs are functions of that sub-matrix alone.  A
 * round of outlier removal -- computePca, drop the samples far out on a leading axis, computePca again -- therefore costs one
 * gather of S (8 m^2 bytes of traffic) plus one pcoa_compute, not one more pass over every variant.
 *
 * pcoa_create_subset: a NEW full engine over n_keep samples, on src's device and with src's create flags, whose S is
 *   S_new(a, b) = S_src(keep[a], keep[b]).
 *   keep:   host array of n_keep >= 1 STRICTLY INCREASING indices in [0, pcoa_n_samples(src)); consumed when the call returns.
 *           NULL, n_keep < 1, an index out of range, an unsorted or a repeated index: PCOA_ERR_INVALID_ARG, found on the host
 *           before any device work.
 *   src:    an ordinary full engine (pcoa_create, or the result of this call).  A strip owner or an operator ctx:
 *           PCOA_ERR_STATE.  src is finalized and its input checks are read first (an S that a check has invalidated is never
 *           subset; that error comes back as it would from pcoa_gram_finalize).  src is otherwise unchanged: it may be fed
 *           further, read, subset again or destroyed afterwards.
 *   result: an ordinary engine in every respect -- pcoa_compute, pcoa_gram_read*, pcoa_center_read_f64, pcoa_gram_reduce_from,
 *           pcoa_create_subset again and further pcoa_accumulate_* calls over n_keep samples all work on it.  It carries src's
 *           bound of the int32 entries (what the int64 fold and the int32 reductions go by) and src's gram_variants; where src
 *           has an int64 part that is gathered too and then narrowed back into the int32 matrix if every kept entry fits
 *           (pcoa_timings.narrowed_to_int32), as every other int64 hand-over is.  Timings: subset_seconds / subset_bytes.
 *   memory: the peak is S of src PLUS S of the result (4 n^2 + 4 n_keep^2 bytes; 12 of each where src has an int64 part).
 *           Allocation failure: PCOA_ERR_OUT_OF_MEMORY, *out = NULL, src usable.  An in-place or masked form for an S that
 *           fills the HBM does not exist.
 * Errors are reported on src (pcoa_last_error(src)); with src == NULL or out == NULL, on pcoa_last_error(NULL).  On any
 * failure *out = NULL.  Synchronising on both engines.
 * Extends: computePca (VariantsPca.scala:198-231) to a sub-cohort of the matrix getSimilarityMatrix built, the step a
 * smartpca-style outlier loop repeats. */
int pcoa_create_subset(pcoa_ctx** out, pcoa_ctx* src, const int32_t* keep, int32_t n_keep);

/* ---- screening a stored S for duplicate and related sample pairs ------------------------------------------------------------
 * S(i, i) = d_i is the number of variants sample i carries, S(i, j) the number two samples share, so
 * S(i, j) / (d_i + d_j - S(i, j)) is the Jaccard index of their carrier sets: 1 for a duplicate, high for first-degree relatives.
 * The rule, with S(i, j) the TOTAL entry (the int32 matrix plus the int64 part where the ctx has one) and U = d_i + d_j - S(i, j):
 *   the pair (i, j), i < j, is REPORTED iff U > 0 and (double)S(i, j) >= min_jaccard * (double)U
 * -- one IEEE fp64 multiplication and one comparison (nothing to contract), every integer below 2^53: the same expression in
 * numpy (variants_pca.related_pairs_rule) reports the same pairs, bit for bit.
 *
 * pcoa_similar_pairs: one memory-bound screen of the upper triangle of S on the device (count, scan, write: csrc/pairs.hip).
 *   ctx:     an ordinary full engine: from pcoa_create, a subset, or one with a loaded or reduced S.  A strip owner or an operator
 *            ctx: PCOA_ERR_STATE, the message names the kind of ctx, the ctx stays usable.  ctx is finalized and its input checks
 *            are read first (an S that a check has invalidated is never screened; that error comes back as it would from
 *            pcoa_gram_finalize).
 *   min_jaccard: finite, in (0, 1].
 *   out_pairs / capacity: receives the first min(n_found, capacity) reported pairs in increasing (i, j) order; entries behind
 *            them are not touched.  capacity == 0 is a count-only call (out_pairs may be NULL).  n_found > capacity is not an
 *            error: the caller compares the two.
 *   *n_found_out: the number of pairs the rule reports -- always the full count.
 *   out_diag: N entries d_0 .. d_{N-1}, or NULL.
 *   PCOA_ERR_INVALID_ARG, found on the host before any device work: ctx or n_found_out NULL, capacity < 0, capacity > 0 with
 *            out_pairs NULL, min_jaccard not finite or outside (0, 1].
 *   memory:  N ceil(N / 1024) int32 counts, 2 N + 2 int64 and min(capacity, N (N - 1) / 2) pairs on the device, all allocated
 *            before the first launch and freed before the call returns; PCOA_ERR_OUT_OF_MEMORY leaves the ctx usable.
 * Content and order are a function of S and min_jaccard alone: not of the grid, the CU count or how S was accumulated (no
 * floating-point atomics; the list is not sorted, it is written in order).  S is unchanged and the ctx computes the same bits
 * afterwards.  Synchronising.  Statistics: pcoa_get_pairs_stats.
 * Extends: computePca (VariantsPca.scala:198-231) by the screen every genetics PCA pipeline runs before the decomposition, over
 * the matrix getSimilarityMatrix built (:182-191); with pcoa_create_subset: screen, drop one of each pair, decompose
 * S[kept, kept], no variant read twice. */
typedef struct pcoa_pair { int32_t i, j; int64_t shared; } pcoa_pair;   /* i < j, shared = S(i, j) */
int pcoa_similar_pairs(pcoa_ctx* ctx, double min_jaccard, pcoa_pair* out_pairs, int64_t capacity, int64_t* n_found_out,
                       int64_t* out_diag /* N entries or NULL */);

/* What pcoa_similar_pairs did on THIS engine, cumulative since pcoa_create / pcoa_reset_timings.  (A struct of its own, like
 * pcoa_reduce_peers_stats: the layout and the size of pcoa_timings are held fixed by its readers.)  It grows at its end;
 * out_size = sizeof of the struct the caller compiled against.  Synchronising, like pcoa_get_timings. */
typedef struct pcoa_pairs_stats {
  double pairs_seconds;   /* HIP-event time of the screens: diagonal, count, scans, write                                     */
  int64_t pairs_bytes;    /* bytes of S the scan kernels read: the count pass's (band, tile) blocks above the diagonal plus the
                             (row, tile) cells the write pass read again; 4 per entry, 12 where S has an int64 part           */
  int64_t pairs_calls;
} pcoa_pairs_stats;
int pcoa_get_pairs_stats(pcoa_ctx* ctx, pcoa_pairs_stats* out, size_t out_size);

/* ---- principal coordinates of a normalised similarity, evaluated on the fly from S -------------------------------------------
 * S(i, j) scales with how many variants each of the two samples carries, d_i = S(i, i): samples with more non-reference calls
 * (coverage, caller, array, ancestry) have uniformly larger rows, and after centring a leading axis tracks d_i.  The remedy is to
 * decompose a normalised similarity K: classical PCoA on the distance sqrt(1 - Jaccard) is the eigenproblem of 1/2 J K J, the
 * vectors of the centred K with the eigenvalues halved.  K is never in memory: the mat-vecs, the row sums and the centring
 * evaluate it per entry from the integer S (csrc/measure.hip).  The rule, with s = S(i, j) the TOTAL entry (the int32 matrix plus
 * the int64 part where the ctx has one), in IEEE fp64 with no contraction:
 *   PCOA_SIMILARITY_SHARED   K = (double)s                                                 what the reference decomposes
 *   PCOA_SIMILARITY_JACCARD  U = d_i + d_j - s (integer);  K = U > 0 ? (double)s / (double)U : 0.0        one division
 *   PCOA_SIMILARITY_COSINE   q_i = d_i > 0 ? 1.0 / sqrt((double)d_i) : 0.0;  K = ((double)s * q_i) * q_j      (Ochiai)
 *   centring (all three)     r_i = sum_j K(i, j);  mm = (sum_i r_i) / N / N;  B(i, j) = ((K(i, j) - r_i / N) - r_j / N) + mm
 * -- variants_pca.similarity_measure / centred_measure are the numpy statement.  Jaccard's diagonal is 1 where d_i > 0; a sample
 * that carries nothing has a zero row and column under both measures and is not counted in nonzero_rows.  Both are positive
 * semi-definite (Tanimoto, cosine), so pcoa_compute's selection by |lambda| applies unchanged.  The upper-triangle mat-vec
 * evaluates K(i, j) once, for i <= j, and uses it for both triangles.
 *
 * pcoa_set_similarity: what pcoa_compute decomposes from now on.  A property of how the ctx DECOMPOSES S, not of how it
 *   accumulates it: it may be set at any time (before the first variant, after a reduction or a load), survives pcoa_reset as the
 *   create flags do, and the result of pcoa_create_subset inherits it.  Nothing of a centring is kept between calls, so the next
 *   pcoa_compute / pcoa_center_read_f64 starts from the row sums of the measure then set.
 *   With JACCARD or COSINE set: pcoa_compute decomposes the measure's B (Lanczos, band Lanczos, the Householder fallback; the
 *   timings, matvec_form, eig_method and lanczos_steps describe the path as before); pcoa_center_read_f64 returns the measure's B,
 *   its fp64 row sums r_i, mm and nonzero_rows = #{r_i > 0}; pcoa_debug_centred_matvec multiplies by the measure's B, forms 0, 1,
 *   2 with the preconditions it has.  pcoa_project with such a ref: PCOA_ERR_STATE (not built).  pcoa_similar_pairs, pcoa_gram_*,
 *   pcoa_gram_reduce_* and pcoa_create_subset's gather never look at the measure.  With SHARED (the default) every call is what it
 *   was, bit for bit.
 *   kind:  an unknown kind: PCOA_ERR_INVALID_ARG.  ctx NULL: PCOA_ERR_INVALID_ARG on pcoa_last_error(NULL).
 *   ctx:   a strip owner or an operator ctx takes SHARED only; any other kind: PCOA_ERR_STATE, the message names the kind of ctx,
 *          the ctx stays usable (measures over strips or over the implicit operator are not built).
 *   memory: N int64 (and N doubles for the cosine), allocated by the first centring under a measure.
 * pcoa_get_similarity: *kind_out = the kind set (PCOA_SIMILARITY_SHARED after create).  No device work in either call.
 * Extends: computePca (VariantsPca.scala:198-231), which centres and decomposes the shared counts only, by the normalised
 * similarities a principal COORDINATES analysis is usually run on. */
#define PCOA_SIMILARITY_SHARED  0   /* default: today's behaviour, bit for bit */
#define PCOA_SIMILARITY_JACCARD 1
#define PCOA_SIMILARITY_COSINE  2
int pcoa_set_similarity(pcoa_ctx* ctx, int32_t kind);
int pcoa_get_similarity(const pcoa_ctx* ctx, int32_t* kind_out);

/* ---- the pairwise-complete similarity: S normalised by the jointly called variants ------------------------------------------
 * "A missing call carries nothing": a PLINK .bed code 01 is decoded as a non-carrier, so a sample with 20 % missing genotypes
 * has a uniformly smaller row of S, and after centring a leading axis tracks call rate instead of ancestry.  The remedy every
 * GRM / IBS tool applies: divide each pair's shared count by the number of variants at which BOTH samples were called.  With
 * s = S(i, j) the TOTAL entry of this ctx (the int32 matrix plus the int64 part where there is one), Q the finalized S of a
 * second ordinary engine -- the COMPANION, fed the bitsets of the missing calls -- and V the number of variants fed:
 *   c_i     = V - Q(i, i)                       (int64; the variants at which sample i is called)
 *   M(i, j) = c_i + c_j - V + Q(i, j)           (int64; both called)
 *   K(i, j) = M > 0 ? (double)s / (double)M : 0.0                          one IEEE fp64 division, no contraction
 *   centring  r_i = sum_j K(i, j);  mm = (sum_i r_i) / N / N;  B(i, j) = ((K(i, j) - r_i / N) - r_j / N) + mm
 * -- variants_pca.call_complete_measure / centred_measure are the numpy statement; nonzero_rows = #{r_i > 0}.  K is never in
 * memory: the mat-vecs, the row sums and the centring evaluate it per entry from the two integer matrices (csrc/complete.hip).
 * Unlike Jaccard and cosine this K is NOT positive semi-definite in general (on the test cohorts the most negative eigenvalue of
 * B is about 1 % of lambda_1); pcoa_compute selects by |lambda| as it always has.
 *
 * pcoa_set_call_companion: binds `missing` as ctx's companion with V = n_variants; missing == NULL unbinds.  From then on
 *   pcoa_compute, pcoa_center_read_f64 and pcoa_debug_centred_matvec (forms 0, 1, 2 with the preconditions they have) use the
 *   rule.  Like the measure it is a property of how the ctx DECOMPOSES, not of how it accumulates: it may be set at any time and
 *   survives pcoa_reset; the caller binds again when V changes.  At each centring the companion is finalized and its input
 *   checks are read; an error of the companion is reported on ctx and says where it came from.  With no companion bound every
 *   call returns the bits it returned before.  pcoa_similar_pairs, pcoa_gram_* and the reductions never look at the binding.
 *   Refused before any device work, the ctx stays usable:
 *     PCOA_ERR_INVALID_ARG  ctx NULL (on pcoa_last_error(NULL)), missing == ctx, differing N, n_variants < 0
 *     PCOA_ERR_STATE        either ctx is a strip owner or an operator ctx; the two are on different devices; the companion
 *                           itself has a companion; ctx has a Jaccard / cosine measure set (and pcoa_set_similarity(JACCARD |
 *                           COSINE) on a bound ctx is refused the same way: the combination is not built)
 *   At centring time: a companion with an int64 part: PCOA_ERR_STATE (not built; ctx's own int64 part IS supported, in the row
 *   form); Q(i, i) > V for some i: PCOA_ERR_INVALID_ARG ("n_variants is smaller than a sample's missing count").
 *   pcoa_project with a bound ref: PCOA_ERR_STATE (not built).
 *   pcoa_create_subset(src) with src bound: the result gets a companion of its own, Q[keep, keep] with the same V, gathered by
 *   the same kernel, OWNED by the result and destroyed with it (or when the result is bound again or unbound).
 *   Destroying a caller-owned companion that is still bound is the caller's error: unbind first.
 *   memory: N int64, allocated by the first centring under a binding.
 * pcoa_get_call_companion: *missing_out = the companion bound (NULL: none), *n_variants_out = its V (0: none); either may be NULL.
 *
 * pcoa_accumulate_plink_bed_calls: pcoa_accumulate_plink_bed -- the same arguments, chunking, staging slots, lifetime rules and
 *   PCOA_BED_HOST_ASYNC behaviour -- feeding TWO engines from one read of the rows: host rows cross the link once, one decode
 *   kernel reads each raw row once and writes the carrier bitsets (bit for bit those of pcoa_accumulate_plink_bed) into ctx and
 *   the missing bitsets (code 01, samples >= N masked) into `missing`.  The order between the two engines' streams is kept by
 *   events; there is no host wait beyond the existing call's.  `missing` must be an ordinary packed-operand full engine on
 *   ctx's device with ctx's N (else PCOA_ERR_INVALID_ARG); it need not be bound.  Callers that hold bitsets already feed the
 *   companion through pcoa_accumulate_bits.
 * Extends: hasVariation (VariantsPca.scala:56-60), for which a missing call is a non-carrier, and computePca
 * (VariantsPca.scala:198-231), which centres and decomposes the shared counts only, by the pairwise-complete normalisation. */
int pcoa_set_call_companion(pcoa_ctx* ctx, pcoa_ctx* missing, int64_t n_variants);
int pcoa_get_call_companion(const pcoa_ctx* ctx, pcoa_ctx** missing_out, int64_t* n_variants_out);
int pcoa_accumulate_plink_bed_calls(pcoa_ctx* ctx, pcoa_ctx* missing, const uint8_t* bed_rows, int64_t n_variants,
                                    int64_t row_bytes, int ref_is_a1, int is_device_ptr);

/* ---- KING-robust kinship screen from PLINK genotypes -----------------------------------------------------------------------------
 * The carrier-Jaccard screen (pcoa_similar_pairs) depends on allele frequencies: on a cohort with population structure an
 * unrelated pair of one population can share more carriers than a parent and a child.  The KING-robust coefficient does not.
 * Per variant every sample is in exactly one class by its .bed code: R = 00 (hom A1), M = 01 (missing), H = 10 (het),
 * A = 11 (hom A2); KING is symmetric in the two alleles, so there is no ref_is_a1.  Five PLANES -- bitsets of one class, one bit
 * per sample and variant -- are accumulated into five ordinary full engines, in this order:
 *   PCOA_KING_HET 0: H    PCOA_KING_MISSING 1: M    PCOA_KING_HET_OR_MISSING 2: H u M    PCOA_KING_HOM_A1 3: R    PCOA_KING_HOM_A2 4: A
 * With G_p the finalized S of plane p and lower-case letters its diagonal (h_i = G_H(i, i), hm_i = G_HM(i, i), ...):
 *   V        = r_i + a_i + hm_i                                          (int64; must be the same for every i)
 *   hethet   = G_H(i, j)                                                 (both heterozygous)
 *   s_hm     = G_HM(i, j) - G_H(i, j) - G_M(i, j)                        (one het, the other missing; H, M disjoint)
 *   het_sum  = h_i + h_j - s_hm                                          (hets of i where j is called + hets of j where i is called)
 *   ibs0     = (V - hm_i - hm_j + G_HM(i, j)) - G_R(i, j) - G_A(i, j)    (opposite homozygotes: the complement of H u M is R u A)
 *   num      = hethet - 2 ibs0                                           (int64, may be negative)
 *   the pair (i, j), i < j, is REPORTED iff het_sum > 0 and (double)num >= min_kinship * (double)het_sum
 *   kinship  = (double)num / (double)het_sum                             (hosts only; the library returns the integers)
 * -- one IEEE fp64 multiplication and one comparison, every integer below 2^53: variants_pca.king_counts / king_pairs_rule are
 * the numpy statement and report the same pairs, bit for bit.  num / het_sum is the KING-robust estimator over the jointly
 * called sites.  The rule above is the contract, not any tool's output.
 *
 * The planes: the caller creates five engines with pcoa_create (the same N, the same device, packed-operand) and owns them.
 *   Refused before any device work by both calls, reported on planes[0] (on pcoa_last_error(NULL) where planes or planes[0] is
 *   NULL), PCOA_ERR_INVALID_ARG: a NULL array or entry, a ctx that appears twice, differing N or device, a strip owner or an
 *   operator ctx, a PCOA_FLAG_GRAM_F32_MFMA engine.
 * pcoa_accumulate_plink_bed_king: pcoa_accumulate_plink_bed -- the same rows, chunking through the staging slots of planes[0],
 *   lifetime rules and PCOA_BED_HOST_ASYNC behaviour -- feeding the FIVE planes from one read of the rows: host rows cross the
 *   link once, one decode kernel reads each raw row once and writes the five bitset rows (samples >= N masked in every plane:
 *   the padding codes of a row's last byte are 00 and would land in R), plane p's rows go into plane p on its own stream.  The
 *   order between the streams is kept by events (one "decoded" event the planes 1 - 4 wait for, one "read" event per plane that
 *   planes[0]'s stream waits for before the next decode); there is no host wait beyond the existing call's.  A chunk holds at
 *   most 2^17 rows, and fewer where five plane buffers of that many rows would pass 1 GiB together.  An error of a plane is
 *   reported on planes[0] and names the plane.
 * pcoa_king_pairs: finalizes the five planes and reads their input checks (an invalidated S is never screened), then one
 *   memory-bound screen of the upper triangle of the five matrices on planes[0]'s stream (diagonal, count, scan, write:
 *   csrc/king.hip).
 *   min_kinship: finite, in (0, 0.5].
 *   out_pairs / capacity / *n_found_out: as pcoa_similar_pairs -- the first min(n_found, capacity) pairs in increasing (i, j)
 *            order, the rest untouched; capacity == 0 counts only; *n_found_out is always the full count.
 *   *n_variants_out: V, or NULL.  out_het: N entries h_0 .. h_{N-1}, or NULL.
 *   PCOA_ERR_INVALID_ARG before any device work: n_found_out NULL, capacity < 0, capacity > 0 with out_pairs NULL, min_kinship
 *            not finite or outside (0, 0.5].
 *   PCOA_ERR_STATE: a plane has an int64 part (more than 2^30 variants; not built).
 *   PCOA_ERR_INVALID_ARG behind the kernels, the message names the check: the planes were not fed the same rows -- V differs
 *            between samples, or some ibs0, het_sum or s_hm is negative.  Nothing is written to the outputs then.
 *   memory:  FIVE N x N int32 matrices (plus the main engine's where a PCA runs beside the screen): at N = 100,000 that is
 *            200 GB (+ 40 GB).  The screen itself: N ceil(N / 1024) int32 counts, 3 N + 5 int64 and min(capacity, N (N - 1) / 2)
 *            pairs of 32 bytes, allocated before the first launch and freed before the call returns.
 * Content and order are a function of the five matrices and min_kinship alone.  The matrices are unchanged and the planes stay
 * usable, also after an error.  Synchronising.  Statistics (on planes[0]): pcoa_get_king_stats.
 * Not built: strips, operator engines, several devices, an int64 part in a plane, VCF input (carriers only), the
 * min-heterozygosity ("between-family") variant, IBD-segment or PI_HAT estimates.
 * Extends: computePca (VariantsPca.scala:198-231) by the relatedness screen the field runs before a PCA (PLINK 2 --king-cutoff,
 * KING, SNPRelate), over Gram matrices built the way getSimilarityMatrix (:182-191) builds S; with pcoa_create_subset on the main
 * engine: screen, drop one of each pair, decompose S[kept, kept]. */
#define PCOA_KING_HET            0
#define PCOA_KING_MISSING        1
#define PCOA_KING_HET_OR_MISSING 2
#define PCOA_KING_HOM_A1         3
#define PCOA_KING_HOM_A2         4
#define PCOA_KING_PLANES         5
typedef struct pcoa_king_pair { int32_t i, j; int64_t hethet, ibs0, het_sum; } pcoa_king_pair;   /* i < j; 32 bytes */
int pcoa_accumulate_plink_bed_king(pcoa_ctx* const* planes /* [PCOA_KING_PLANES] */, const uint8_t* bed_rows,
                                   int64_t n_variants, int64_t row_bytes, int is_device_ptr);
int pcoa_king_pairs(pcoa_ctx* const* planes, double min_kinship, pcoa_king_pair* out_pairs, int64_t capacity,
                    int64_t* n_found_out, int64_t* n_variants_out /* V or NULL */, int64_t* out_het /* N x h_i or NULL */);

/* What pcoa_king_pairs did, cumulative on planes[0] since pcoa_create / pcoa_reset_timings (a struct of its own, like
 * pcoa_pairs_stats; it grows at its end; out_size = sizeof of the struct the caller compiled against).  Synchronising. */
typedef struct pcoa_king_stats {
  double king_seconds;   /* HIP-event time of the screens: diagonal, count, scans, write                                        */
  int64_t king_bytes;    /* bytes of the five matrices the scan kernels read: 20 per entry of the count pass's (band, tile)
                            blocks above the diagonal and of the (row, tile) cells the write pass read again                    */
  int64_t king_calls;
} pcoa_king_stats;
int pcoa_get_king_stats(pcoa_ctx* plane0, pcoa_king_stats* out, size_t out_size);

/* ---- the KING-robust kinship screen on the resident 2-bit store of a GRM ctx ---------------------------------
 * K is standardised by cohort-wide allele frequencies, so on a cohort with population structure pcoa_grm_pairs inflates
 * within-population pairs; the screen the field runs in front of a genotype PCA is plink2 --king-cutoff.  These calls apply
 * pcoa_king_pairs' rule to the store a GRM ctx already holds: no plane engines, no N x N matrix, no second pass over the
 * fileset, and the counted rows can be the QC'd, LD-pruned ones.  The rule, on genotype classes: at a row v of the store sample i
 * is H (heterozygous), R or A (the two homozygotes: KING is symmetric in them, so the store's single coding needs no undoing) or
 * M (not called; every padding slot is M); C = R u H u A.  Over the COUNTED rows, all exact integers:
 *   hethet(i, j)  = sum_v H_vi H_vj
 *   ibs0(i, j)    = sum_v (R_vi A_vj + A_vi R_vj)
 *   het_sum(i, j) = sum_v (H_vi C_vj + C_vi H_vj)
 *   the pair (i, j), i < j, is REPORTED iff het_sum > 0 and (double)(hethet - 2 ibs0) >= min_kinship * (double)het_sum
 * (variants_pca.py's grm_king_rule / grm_king_pairs_rule are the numpy statement).  The diagonal follows the same expressions:
 * hethet(i, i) = h_i, ibs0(i, i) = 0, het_sum(i, i) = 2 h_i.  Off the diagonal these are the integers pcoa_king_pairs derives from
 * five plane engines fed the same .bed rows, so the records are the same bytes.
 *   rows_kind: PCOA_GRM_ROWS_ALL (every row of the store; either GRM kind) or PCOA_GRM_ROWS_USED (the rows with used_v under
 *           min_maf, the filters and an installed LD mask; PCOA_ERR_STATE on a study ctx), as pcoa_grm_sample_counts.
 *
 * pcoa_grm_king_block: the rectangle [row0, row0 + rows) x [col0, col0 + cols) of the three counts, int32, row-major; any output
 *   may be NULL, not all three; host memory, or device memory of the ctx's device with is_device_ptr.  Four int8 products on
 *   the matrix cores, fed from the store words (csrc/grm_king.hip), one launch per segment of the store.  Integers: any cut of a
 *   rectangle gives the same numbers, (i, j) and (j, i) are equal.  Synchronising.
 * pcoa_grm_king_pairs: walks the upper triangle in bands of band_rows rows (a multiple of 64; 0 = 1,024): the band's counts
 *   [r0, r0 + band_rows) x [64 floor(r0 / 64), N) go into the ctx's workspace, then count, row scan, offset scan from the running
 *   total in device memory and the ordered write: one launch chain per band, no host synchronisation between bands.  Pairs come
 *   out in increasing (i, j) order without a sort.
 *   min_kinship: finite, in (0, 0.5].
 *   out_pairs / capacity / *n_found_out: as pcoa_similar_pairs -- the first min(n_found, capacity) pairs, entries behind them
 *           untouched; capacity 0 is the count-only call; *n_found_out is always the full count.
 *   *n_rows_out: the counted rows, or NULL.  out_het: N entries h_i over the counted rows (from the bands' diagonal), or NULL.
 *   Synchronising.  Content and order are a function of the store, the counted rows and min_kinship alone.
 * Nothing writes the store: pcoa_compute returns the same bits before and after.
 *   PCOA_ERR_INVALID_ARG, found on the host before any device work: ctx NULL (pcoa_last_error(NULL)), n_found_out NULL, an
 *           unknown rows_kind, band_rows negative or not a multiple of 64, capacity < 0, capacity > 0 with out_pairs NULL, a
 *           min_kinship that is not finite or outside (0, 0.5], a rectangle that leaves [0, N)^2, all three outputs NULL.
 *   PCOA_ERR_STATE, the ctx stays usable: a ctx without a genotype store (the message names its kind), PCOA_GRM_ROWS_USED on a
 *           study ctx, no counted row, 2^30 or more counted rows (het_sum <= 2 V must fit int32: the plane path's limit).
 *   memory: 3 * band_rows * 64 ceil(N / 64) int32 (pcoa_grm_king_block with host outputs: one rows * cols int32 per output) in the
 *           lazily grown buffer pcoa_grm_block uses; the (row, tile) counts, the row offsets, h and min(capacity, N (N - 1) / 2)
 *           records for the length of the call, all allocated before the first launch.  PCOA_ERR_OUT_OF_MEMORY leaves the ctx
 *           usable.
 * Not built: the min-heterozygosity ("between-family") variant, PI_HAT / IBD estimates, a threshold fused into the count kernel's
 * epilogue, skipping the tiles of a band's first block below the diagonal, a split along variants for small N, multi-GPU,
 * JNI / Scala natives. */
int pcoa_grm_king_block(pcoa_ctx* ctx, int32_t rows_kind, int32_t row0, int32_t rows, int32_t col0, int32_t cols,
                        int32_t* out_hethet, int32_t* out_ibs0, int32_t* out_het_sum /* [rows][cols] each; any may be NULL, not all */,
                        int is_device_ptr);
int pcoa_grm_king_pairs(pcoa_ctx* ctx, int32_t rows_kind, double min_kinship, int32_t band_rows /* 0: 1,024; multiple of 64 */,
                        pcoa_king_pair* out_pairs, int64_t capacity, int64_t* n_found_out,
                        int64_t* n_rows_out /* counted rows, or NULL */, int64_t* out_het /* N x h_i, or NULL */);

/* What the two calls did on THIS engine, cumulative since pcoa_create_grm / pcoa_reset_timings.  (A struct of its own, like
 * pcoa_grm_pairs_stats.)  It grows at its end; out_size = sizeof of the struct the caller compiled against.  Synchronising. */
typedef struct pcoa_grm_king_stats {
  double grm_king_seconds;          /* HIP-event time of every launch of the calls: the count kernel and the screen            */
  double grm_king_screen_seconds;   /* of which the screen's count, scan and write kernels                                    */
  int64_t grm_king_calls;           /* pcoa_grm_king_pairs calls                                                              */
  int64_t grm_king_bands;
  double grm_king_macs;             /* int8 multiply-adds the count kernel issued: 4 products * tile rows * tile columns of the
                                       64 x 64 tiles launched * store rows rounded up to 32 per segment                        */
  int64_t grm_king_bytes;           /* bytes of the bands the screen's count and write kernels read: 12 per entry              */
  int64_t grm_king_block_calls;     /* pcoa_grm_king_block calls                                                              */
} pcoa_grm_king_stats;
int pcoa_get_grm_king_stats(pcoa_ctx* ctx, pcoa_grm_king_stats* out, size_t out_size);

/* ---- PC-Relate kinship on the resident 2-bit store of a GRM ctx ------------------------------------------------
 * pcoa_grm_pairs thresholds K, which is standardised by cohort-wide frequencies and inflates every pair that shares ancestry;
 * pcoa_grm_king_pairs needs no frequencies but is biased downwards for relatives whose ancestry differs.  PC-Relate (Conomos et al.
 * 2016, GENESIS pcrelate) adjusts the kinship for the ancestry the axes found: the dosages are regressed on an intercept and the
 * leading axes, the fitted value is the individual's own allele frequency, and the kinship is the residual covariance over the
 * individual-specific variances.  c_iv, g_iv, n_v, mu_v, used_v are pcoa_create_grm's.  Inputs: n_cov covariates, 1 <= n_cov <= 9
 * (an intercept and up to 8 axes), as two host matrices basis[n_cov][N] and hat[n_cov][N].
 *   fit        S_c     = sum_i hat[c][i]                           on the host, i ascending, fp64
 *              beta_vc = (A hat_c)_v + mu_v * S_c                  (A hat_c)_v: pass 1 of the operator applied to hat_c (A = g - mu c),
 *                                                                  the sample groups' partials added in group order
 *              = sum_i hat[c][i] * (c_iv ? g_iv : mu_v): missing calls mean-imputed; defined for EVERY row of the store
 *   frequency  e_iv  = beta_v0 * basis[0][i];  for c = 1 .. n_cov-1:  e_iv = e_iv + beta_vc * basis[c][i];   mu_iv = 0.5 * e_iv
 *              every product and sum rounded on its own, no contraction, in exactly this order
 *   operands   for a threshold t in [0, 0.5), one_minus_t = 1.0 - t:
 *              m_iv = used_v and c_iv and mu_iv > t and mu_iv < one_minus_t
 *              a_iv = m_iv ? (double)g_iv - e_iv : 0.0          b_iv = m_iv ? sqrt(mu_iv * (1.0 - mu_iv)) : 0.0   (correctly rounded)
 *   kinship    num(i,j) = sum_v a_iv a_jv    den(i,j) = sum_v b_iv b_jv    n(i,j) = sum_v m_iv m_jv (exact integer)
 *              phi(i,j) = den(i,j) > 0 ? num(i,j) / (4.0 * den(i,j)) : 0.0
 * The diagonal follows the same expression; the inbreeding coefficient is 2 phi(i,i) - 1, the caller's to compute.  The estimator
 * is symmetric in the two alleles.  variants_pca.py's pcrelate_hat_rule, grm_pcrelate_isaf_rule and grm_pcrelate_rule are the
 * numpy statements.  As pcoa_grm_block: (i, j) and (j, i) have the same bits (nothing scales an operand, so there are no tile
 * modes); an entry's bits depend on the store, the fit, used_v, t and (i, j) only, not on the rectangle; no atomics: additions
 * into an entry happen in the order of the variants' indices in their segment, four at a time (csrc/grm_pcrelate.hip, three fp64
 * products on v_mfma_f64_16x16x4_f64 with the operands formed in registers; instantiated for 1, 3, 5 and 9 covariates, a fit with
 * another count is padded with beta = 0, basis = 0, which changes no bit of e but the sign of a zero, and a zero is masked).
 *
 * pcoa_pcrelate_hat: pure host arithmetic, no ctx, no device: hat = (basis basis^T)^-1 basis.  G[c][c'] = sum_i basis[c][i] *
 *   basis[c'][i], i ascending, each product rounded, then added; then the square-root-free L D L^T of pcoa_grm_project_lsq,
 *   literally that sequence; then its forward / diagonal / backward solve per sample column.  PCOA_ERR_INVALID_ARG, the message
 *   through pcoa_last_error(NULL): n_cov outside [1, 9], n < n_cov, a non-finite entry, a pivot <= 2^-40 * G[c][c] (collinear
 *   covariates; c is named).
 * pcoa_grm_pcrelate_fit: leaves beta [V][n_cov] and the basis resident on the ctx's device; replaces an earlier fit; the counts and
 *   weights are recomputed if they are not resident.  The fit depends on the store and the two matrices only -- not on min_maf,
 *   the filters or the LD mask, which enter through used_v when a block is asked for.  hat need not be a pseudo-inverse.
 *   pcoa_accumulate_plink_bed and pcoa_reset drop the fit; a subset does not inherit it; pcoa_destroy frees it.  Synchronising.
 * pcoa_grm_pcrelate_beta: beta of the rows [first_variant, first_variant + n_variants), host [n_variants][n_cov].
 * pcoa_grm_pcrelate_isaf: mu_iv of every sample and row of the window, unmasked, host [n_variants][N] (GENESIS calls it ISAF).
 * pcoa_grm_pcrelate_block: any rectangle of phi and / or of n, row-major; host memory, or device memory of the ctx's device with
 *   is_device_ptr; either output may be NULL, not both.  Memory and error conventions are pcoa_grm_block's.  Synchronising.
 * pcoa_grm_pcrelate_pairs: pcoa_grm_pairs' walk of the upper triangle: bands of band_rows rows (a multiple of 64; 0 = 1,024) x
 *   [64 floor(r0 / 64), N) sit in the buffer pcoa_grm_block grows -- num, den and n side by side -- one launch chain per band, no
 *   host synchronisation between bands; the screen is pcoa_grm_pairs' count / scan / write.  The pair (i, j), i < j, is reported
 *   iff phi(i, j) >= cutoff on the very bits pcoa_grm_pcrelate_block returns; records are pcoa_grm_pair {i, j, k = phi, n = n(i, j)}
 *   in (i, j) order; capacity and *n_found_out as pcoa_similar_pairs; out_diag[i] = phi(i, i), or NULL.  Synchronising.
 *   PCOA_ERR_INVALID_ARG, found on the host before any device work: ctx NULL; fit: NULL matrices, n_cov outside [1, 9], a
 *           non-finite entry; beta / isaf: a window outside the store, NULL out; block: a rectangle that leaves [0, N)^2, both
 *           outputs NULL; block / pairs: maf_threshold not finite or outside [0, 0.5); pairs: cutoff not finite, band_rows negative
 *           or not a multiple of 64, capacity < 0, capacity > 0 with out_pairs NULL, n_found_out NULL.
 *   PCOA_ERR_STATE, the ctx stays usable: not a pcoa_create_grm ctx (the message names its kind), a study ctx, an empty store
 *           (fit), M' = 0 or M' >= 2^31 (block / pairs), no fit on this ctx (beta / isaf / block / pairs; the message says what
 *           dropped it when that was an accumulate or a reset).
 * The inbreeding coefficient's n is n(i, i): read it with pcoa_grm_pcrelate_block's pair counts over diagonal blocks.
 * Not built: k0 / k2 / IBD-sharing estimates and the dominance product; GENESIS' scale = "overall" correction and its small-sample
 * correction; maf.bound.method = "truncate"; more than 8 axes; forming e on the matrix cores; removal by PC-Relate kinship and a
 * second PC-AiR round; a fit inherited by subsets; multi-GPU; JNI / Scala natives. */
int pcoa_pcrelate_hat(int32_t n_cov, int32_t n, const double* basis /* [n_cov][n] */, double* hat_out /* [n_cov][n] */);
int pcoa_grm_pcrelate_fit(pcoa_ctx* ctx, int32_t n_cov, const double* basis, const double* hat /* host [n_cov][N] each */);
int pcoa_grm_pcrelate_beta(pcoa_ctx* ctx, int64_t first_variant, int64_t n_variants, double* out /* host [n_variants][n_cov] */);
int pcoa_grm_pcrelate_isaf(pcoa_ctx* ctx, int64_t first_variant, int64_t n_variants, double* out /* host [n_variants][N] */);
int pcoa_grm_pcrelate_block(pcoa_ctx* ctx, int32_t row0, int32_t rows, int32_t col0, int32_t cols, double maf_threshold,
                            double* out_phi, int32_t* out_pairs /* [rows][cols] each; either may be NULL, not both */,
                            int is_device_ptr);
int pcoa_grm_pcrelate_pairs(pcoa_ctx* ctx, double cutoff, double maf_threshold, int32_t band_rows /* 0: 1,024; multiple of 64 */,
                            pcoa_grm_pair* out_pairs, int64_t capacity, int64_t* n_found_out, double* out_diag /* N, or NULL */);

/* What the PC-Relate calls did on THIS engine, cumulative since pcoa_create_grm / pcoa_reset_timings.  (A struct of its own, like
 * pcoa_grm_pairs_stats.)  It grows at its end; out_size = sizeof of the struct the caller compiled against.  Synchronising. */
typedef struct pcoa_grm_pcrelate_stats {
  int64_t grm_pcrelate_fits;            /* pcoa_grm_pcrelate_fit calls                                                         */
  int64_t grm_pcrelate_block_calls;     /* pcoa_grm_pcrelate_block calls                                                       */
  int64_t grm_pcrelate_pairs_calls;     /* pcoa_grm_pcrelate_pairs calls                                                       */
  int64_t grm_pcrelate_bands;
  double grm_pcrelate_fit_seconds;      /* HIP-event time of the fits' launches                                                */
  double grm_pcrelate_dense_seconds;    /* of the dense launches and the division, of both calls                               */
  double grm_pcrelate_screen_seconds;   /* of the screen's count, scan and write kernels                                       */
  double grm_pcrelate_flops;            /* issued fp64 flops: 2 * rows * cols * V per product launched (2 or 3 products)       */
  int64_t grm_pcrelate_bytes;           /* bytes of the bands the screen's count and write kernels read                        */
  int64_t grm_pcrelate_n_cov;           /* NOT cumulative: n_cov of the resident fit, 0 without one (the width of _beta's rows)  */
} pcoa_grm_pcrelate_stats;
int pcoa_get_grm_pcrelate_stats(pcoa_ctx* ctx, pcoa_grm_pcrelate_stats* out, size_t out_size);

/* ---- per-variant loadings of the principal coordinates ---------------------------------------------------------------------
 * Which variants drive each axis (smartpca's SNP weights, PLINK 2's --pca var-wts).  With X the V x N carrier bit matrix and
 * J = I - 11^T / N, the decomposed matrix is B = J S J = (X J)^T (X J), so an eigenpair (u_c, lambda_c) of B is a right singular
 * pair of X J and the matching left singular vector is the loading of every variant on axis c:
 *   w_c = X (J u_c) / sqrt(lambda_c),     w_c[v] = (sum over the carriers i of v of (u_c[i] - mean(u_c))) / sqrt(lambda_c)
 * -- one bit-select-sum per variant and component (csrc/loadings.hip).  The identity holds for PCOA_SIMILARITY_SHARED only.
 *
 * pcoa_loadings_begin: prepares and uploads the vectors once; they stay resident until pcoa_loadings_end or pcoa_destroy, so a
 *   host can stream a cohort through many calls.  A second begin replaces the vectors.
 *   components:  host, [num_pc][n_samples], pcoa_compute's layout; consumed when the call returns.  0 < num_pc <= n_samples.
 *   flags:       PCOA_LOADINGS_CENTRE uses u_c - mean(u_c), the mean being ONE left-to-right fp64 sum divided by N (a function of
 *                the vector alone); PCOA_LOADINGS_UNIT divides the sums by sqrt(eigenvalues[c]) (one correctly rounded square
 *                root on the host, one division per entry).  With flags = 0 the output is the plain sum T[v][c] =
 *                sum_i bit(v, i) components[c][i].  eigenvalues may be NULL without UNIT.
 *   errors:      PCOA_ERR_INVALID_ARG for ctx or components NULL, num_pc outside (0, n_samples], an unknown flag, UNIT with
 *                eigenvalues NULL or an eigenvalue that is <= 0 or not finite; vectors of an earlier begin stay as they were.
 *   Every kind of ctx serves (full engine, strip owner, subset, operator): only n_samples, the device, the stream and the staging
 *   slots of the ctx are used.  Synchronising on the ctx stream.
 * pcoa_loadings_bits: out[v * num_pc + c] for n_variants rows of carrier bitsets in pcoa_accumulate_bits' layout (sample i = bit
 *   i & 31 of word i >> 5, pitch ld_words >= ceil(n_samples / 32)).  Bits of samples >= n_samples and the words behind
 *   ceil(n_samples / 32) are IGNORED, whatever they hold.  bits: host (is_device_ptr = 0; consumed when the call returns) or
 *   device.  out: host (out_is_device = 0; filled when the call returns) or device (the work is queued on the ctx stream; the
 *   device input must stay valid until the next synchronising call).
 * pcoa_loadings_plink_bed: the same for raw .bed rows as they lie in the file, decoded on the device by the rule of
 *   pcoa_accumulate_plink_bed (ref_is_a1 as there; a missing call carries nothing).  is_device_ptr: 0 or 1.
 * pcoa_loadings_operator: the same for rows [first_variant, first_variant + n_variants) of an operator ctx's resident store,
 *   across its segment boundaries.  PCOA_ERR_STATE on a ctx that is not an operator; PCOA_ERR_INVALID_ARG for a range that is
 *   not inside the store.
 *   All three: PCOA_ERR_STATE before pcoa_loadings_begin; PCOA_ERR_INVALID_ARG for a NULL pointer, n_variants < 0, ld_words /
 *   row_bytes too small; the ctx stays usable after every error.  They never modify S or the operator store, and run behind the
 *   accumulation queued on the ctx stream.
 *   Results are reproducible: which additions form entry (v, c), and their order, depend on n_samples alone -- not on num_pc or
 *   on the components that travel with c, not on the number of rows of the call or on the row's place in it, not on the grid or
 *   the CU count, not on where the row came from (host, device, .bed, store).  No floating-point atomics.
 * pcoa_loadings_end: releases the vectors (synchronising); a no-op without a begin.
 * Not built: carrier lists as an input form (a host with lists packs bitsets), the JNI natives.
 * Extends: computePca (VariantsPca.scala:224-246), which stops at the sample coordinates, by the left singular vectors of the
 * same decomposition. */
#define PCOA_LOADINGS_CENTRE 1u   /* use u_c - mean(u_c) */
#define PCOA_LOADINGS_UNIT   2u   /* divide by sqrt(eigenvalues[c]) */
int pcoa_loadings_begin(pcoa_ctx* ctx, int32_t num_pc, const double* components /* [num_pc][n], pcoa_compute's layout */,
                        const double* eigenvalues /* may be NULL without UNIT */, uint32_t flags);
int pcoa_loadings_bits(pcoa_ctx* ctx, const uint32_t* bits, int64_t n_variants, int64_t ld_words, int is_device_ptr,
                       double* out /* out[v * num_pc + c] */, int out_is_device);
int pcoa_loadings_plink_bed(pcoa_ctx* ctx, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes, int ref_is_a1,
                            int is_device_ptr, double* out, int out_is_device);
int pcoa_loadings_operator(pcoa_ctx* ctx, int64_t first_variant, int64_t n_variants, double* out, int out_is_device);
int pcoa_loadings_end(pcoa_ctx* ctx);

/* What the loadings calls did on THIS engine, cumulative since pcoa_create / pcoa_reset_timings.  (A struct of its own, like
 * pcoa_pairs_stats.)  It grows at its end; out_size = sizeof of the struct the caller compiled against.  Synchronising. */
typedef struct pcoa_loadings_stats {
  int64_t loadings_variants;   /* rows the loadings kernels took                                                              */
  int64_t loadings_bytes;      /* bytes of bitsets they read: 4 ceil(N / 32) per row and chunk of <= 8 components             */
  double loadings_seconds;     /* HIP-event time of the loadings kernels (the .bed decode is densify_seconds)                 */
} pcoa_loadings_stats;
int pcoa_get_loadings_stats(pcoa_ctx* ctx, pcoa_loadings_stats* out, size_t out_size);

/* ---- LD pruning of the variants in front of the accumulation ------------------------------------------------------------------
 * The filter every PCA pipeline runs between the allele-frequency filter and the decomposition (PLINK --indep-pairwise,
 * SNPRelate snpgdsLDpruning): a block of correlated variants is otherwise counted many times in S.  Variants arrive in feed order.
 * With n = n_samples, a_v the carrier count of variant v and c_uv = popcount(row_u & row_v), both over samples < n:
 *   D = n c_uv - a_u a_v,   p = a_u (n - a_u),   q = a_v (n - a_v)                      (int64)
 *   exceeds(u, v)  <=>  (double)D * (double)D  >  r2_max * ((double)p * (double)q)          (three fp64 products, no sum)
 * -- r^2 of the two carrier indicators (hasVariation), not of dosages.  The pass is forward and greedy:
 *   a monomorphic variant (a_v = 0 or a_v = n) is removed;
 *   a polymorphic variant v is kept iff no KEPT u with v - window <= u < v, behind the last break, has exceeds(u, v);
 *   a variant that was itself removed blocks nobody.
 * The result depends on the rows, window, r2_max and the breaks only: not on how the rows were split over calls, on where they
 * came from (host, device, .bed), on the grid or on the CU count.  Integer kernels, no atomics (csrc/ld.hip).
 *
 * pcoa_ld_begin: 1 <= window <= PCOA_LD_MAX_WINDOW (in fed variants), 0 <= r2_max <= 1 (NaN refused), flags 0 or
 *   PCOA_LD_ACCUMULATE.  Allocates the pruner's buffers (resident until pcoa_ld_end / pcoa_destroy); a second begin starts over.
 *   Every kind of ctx serves.  After a refused begin an earlier pruner is as it was.
 * pcoa_ld_bits: n_variants rows of carrier bitsets in pcoa_accumulate_bits' layout and pitch; bits of samples >= n_samples and the
 *   words behind ceil(n_samples / 32) are IGNORED, whatever they hold.  bits: host (through the staging slots) or device.
 *   keep_out: host, [n_variants], 1 = kept, may be NULL; n_kept_out: kept rows of THIS call, may be NULL.
 * pcoa_ld_plink_bed: the same for raw .bed rows, decoded on the device by the rule of pcoa_accumulate_plink_bed into a buffer of
 *   the pruner's own.  is_device_ptr: 0 or 1.
 *   The last `window` rows, their counts and their keep flags stay on the device between calls, so a call shorter than the window
 *   is as good as a long one.
 * PCOA_LD_ACCUMULATE: the kept rows of a call are compacted on the device and handed to this ctx's own bitset accumulation as a
 *   device input -- on a full engine, a strip owner or an operator ctx whatever pcoa_accumulate_bits does there (and refused, like
 *   it, on a PCOA_FLAG_GRAM_F32_MFMA engine).  The compacted buffer is the pruner's; its only reader is the accumulation's pre-pass
 *   on the ctx stream, and the kernels that rewrite it are queued on the same stream behind it.  Without the flag nothing is
 *   accumulated (a dry run).
 * pcoa_ld_break: a contig boundary: the carried rows are dropped, the parameters stay.
 * pcoa_ld_end: releases everything (synchronising); a no-op without a begin.  pcoa_reset also drops the carried rows.
 * pcoa_ld_bits / pcoa_ld_plink_bed are SYNCHRONISING on the ctx stream (the kept count of every chunk travels to the host).
 * Errors: PCOA_ERR_STATE before pcoa_ld_begin; PCOA_ERR_INVALID_ARG for a NULL pointer, n_variants < 0, too small a pitch; the ctx
 * and the carried rows stay usable after every error.
 * Not built: windows in base pairs, dosage r^2, PLINK's MAF-ordered removal, windows across engines, the JNI natives.
 * Extends: the filter stage in front of getCallsRdd / getSimilarityMatrix (VariantsPca.scala:96-108 has the AF filter only). */
#define PCOA_LD_MAX_WINDOW 1024
#define PCOA_LD_ACCUMULATE 1u
int pcoa_ld_begin(pcoa_ctx* ctx, int32_t window, double r2_max, uint32_t flags);
int pcoa_ld_bits(pcoa_ctx* ctx, const uint32_t* bits, int64_t n_variants, int64_t ld_words, int is_device_ptr,
                 uint8_t* keep_out /* host, [n_variants], may be NULL */, int64_t* n_kept_out /* may be NULL */);
int pcoa_ld_plink_bed(pcoa_ctx* ctx, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes, int ref_is_a1,
                      int is_device_ptr /* 0 or 1 */, uint8_t* keep_out, int64_t* n_kept_out);
int pcoa_ld_break(pcoa_ctx* ctx);
int pcoa_ld_end(pcoa_ctx* ctx);

/* What the pruner did on THIS engine, cumulative since pcoa_create / pcoa_reset_timings.  It grows at its end; out_size = sizeof
 * of the struct the caller compiled against.  Synchronising. */
typedef struct pcoa_ld_stats {
  int64_t ld_variants;          /* rows seen                                                                                 */
  int64_t ld_kept;              /* rows kept                                                                                 */
  int64_t ld_monomorphic;       /* rows removed because a_v = 0 or a_v = n                                                   */
  int64_t ld_pairs;             /* (earlier row, row) pairs the band kernel evaluated: sum of min(window, rows before it)    */
  double ld_count_seconds;      /* HIP-event time of the carrier-count kernel (it also writes the masked row)                */
  double ld_band_seconds;       /* ... of the band kernel                                                                    */
  double ld_resolve_seconds;    /* ... of the greedy pass                                                                    */
  double ld_compact_seconds;    /* ... of the scan, the gather and the update of the carried rows                            */
} pcoa_ld_stats;
int pcoa_get_ld_stats(pcoa_ctx* ctx, pcoa_ld_stats* out, size_t out_size);

/* ---- layout of S over the engines of one job ------------------------------------------------------------------------
 * FULL: every engine holds a whole N x N partial S (4 N^2 bytes) for its share of the variants; the partials are reduced
 * into engine 0 (peer copies: engine 0 stages one more 4 N^2 matrix when the engines sit on different devices, RCCL
 * otherwise).  STRIPS: engine g holds S[:, col0_g .. col0_g + cols_g) (pcoa_create_strip, 4 N cols_g bytes), is fed EVERY
 * variant, and nothing is reduced; computePca is pcoa_compute_strips.  A strip contraction computes N x cols, both
 * triangles, so the strips together do about twice the matrix-core work per variant of the full layout's upper triangle. */
#define PCOA_LAYOUT_AUTO   0
#define PCOA_LAYOUT_FULL   1
#define PCOA_LAYOUT_STRIPS 2
#define PCOA_LAYOUT_FREE_FRACTION 0.9   /* share of an engine's free bytes the auto rule lets S (+ staging) take */

/* Pure function (no GPU): the layout for N samples on n_engines engines.
 *   request PCOA_LAYOUT_FULL / _STRIPS: that layout.  PCOA_LAYOUT_AUTO with 1 < n_engines <= N: STRIPS exactly when the
 *   full layout does not fit, i.e. when for some engine g   4 N^2 (+ 4 N^2 more on engine 0: the reduce staging)
 *   > PCOA_LAYOUT_FREE_FRACTION * free_bytes[g];  FULL otherwise.  Always FULL with one engine (one strip needs the same
 *   4 N^2 bytes) and when n_engines > N.  The rule is about
 *   memory only -- which layout is faster at a size where both fit has not been measured.
 *   free_bytes[g]: the bytes engine g may use (needed for AUTO only).  Engines that share a device split it: a device with
 *   F free bytes and m engines gives each F / m (the hosts fill it so, from pcoa_device_memory).
 * On STRIPS, col0_out[g] / cols_out[g] (n_engines entries each) receive the column ranges: balanced, every inner cut rounded
 * to the nearest multiple of 256 (the contraction's tile width) when that keeps it strictly between the cut before it and
 * N, and the plain cuts N g / n_engines if some strip would still be empty (the same ranges as strips.strip_ranges).  On FULL
 * they are not written.  PCOA_ERR_INVALID_ARG for a bad request, N or n_engines <= 0, or STRIPS with n_engines > N. */
int pcoa_plan_layout(int32_t n_samples, int32_t n_engines, const int64_t* free_bytes, int32_t request, int32_t* layout_out,
                     int32_t* col0_out, int32_t* cols_out);

/* hipMemGetInfo on device `device_ordinal` (the calling thread's current device is left as it was).  Either pointer may be
 * NULL.  PCOA_ERR_NO_DEVICE / PCOA_ERR_HIP without a usable device. */
int pcoa_device_memory(int32_t device_ordinal, int64_t* free_out, int64_t* total_out);

/* computePca (VariantsPca.scala:198-231) over the strip owners of ONE process; they may share a device or sit on several.
 * owners[0 .. n_owners) must be strip owners of the same N whose ranges, in array order, tile [0, N) without gap or
 * overlap, else PCOA_ERR_INVALID_ARG.  Errors are reported on owners[0] (pcoa_last_error names a failing owner's index).
 *   rowSums (:206-211): each owner's exact int64 column sums land in one N-vector on owners[0] (the lead): in place on the
 *     same device, by peer copy from another; the matrix mean, the non-zero rows and the means rowSums / N follow on the
 *     lead and the means are copied once into every owner's resident centring buffer (as pcoa_strip_set_centering).
 *   principal components (:224-227): the lead's Lanczos (as pcoa_lanczos_with_matvec) with a built-in product: every owner
 *     waits on an event for v (a peer copy when it sits on another device), multiplies its strip on its own stream and
 *     writes its piece straight to y + col0 of the lead's vector (a peer-mapped pointer where peer access exists, else a
 *     local piece + a peer copy); the lead's stream waits on every owner's event.  No host synchronisation per step beyond
 *     the Lanczos iteration's own.  The additions are those of pcoa_strip_matvec_device in the same order: eigenvalues and
 *     components equal, bit for bit, strips.compute_pca_over_strips over the same owners.
 *   N < 32 (below the Lanczos path): the strips are read into one N x N matrix on the host, loaded into a temporary full
 *     engine on the lead's device and solved by pcoa_compute -- the single engine's result by construction.
 * Outputs as pcoa_compute: [num_pc][N] sign-normalised columns, the eigenvalues, the non-zero rows.  Synchronising. */
int pcoa_compute_strips(pcoa_ctx* const* owners, int32_t n_owners, int32_t num_pc, double* out_components,
                        double* out_eigenvalues, int32_t* nonzero_rows_out);

/* Replaces: VariantsPcaDriver.stop (VariantsPca.scala:283-285). */
void pcoa_destroy(pcoa_ctx* ctx);

/* Message of the last error on this ctx (or of the last failed pcoa_create when ctx == NULL).
 * Replaces: the JVM exception message. */
const char* pcoa_last_error(const pcoa_ctx* ctx);

/* Zeroes the accumulated similarity matrix (a fresh getSimilarityMatrix run).  Afterwards the ctx is, for every call that
 * reads S, a ctx fresh from pcoa_create with the same flags: S = 0 in the int32 matrix, NO int64 part whatever S was before
 * (pcoa_timings.gram_i64_live = 0; the matrix is kept as the spare the next fold takes), the bound of the int32 entries zero,
 * buffered or in-flight operands and an LD pruner's carried rows dropped.  What it keeps: the create flags, the similarity
 * measure, the companion binding (and the companion's own S), the stream, every workspace -- and the counters of pcoa_timings,
 * gram_variants among them, which are cumulative since pcoa_create / pcoa_reset_timings and not a statement about S. */
int pcoa_reset(pcoa_ctx* ctx);

int pcoa_n_samples(const pcoa_ctx* ctx);

/* Runs ctx work on a caller-provided hipStream_t (e.g. the host framework's current stream).
 * NULL restores the ctx-owned stream. */
int pcoa_set_stream(pcoa_ctx* ctx, void* hip_stream);

/* Blocks until all queued work of the ctx has finished. */
int pcoa_sync(pcoa_ctx* ctx);

/* Optional.  Allocates NOW what the first calls would otherwise allocate lazily: the operand buffers for accumulate calls
 * of up to `variants_per_call` variants (0 = skip) and the computePca workspace for `num_pc` components (0 = skip), so that
 * no device allocation happens inside a streaming or timed region (a first pcoa_compute is ~4x slower than a later one
 * without it).  Replaces: nothing in the reference -- the JVM allocates its per-partition matrix inside the task
 * (VariantsPca.scala:185); this is the executor warm-up a Spark host would run once per GPU. */
int pcoa_reserve(pcoa_ctx* ctx, int64_t variants_per_call, int32_t num_pc);

/* ---- Gram accumulation: getSimilarityMatrix -------------------------------------------------- */

/* The faithful boundary: exactly what RDD[Seq[Int]] carries (getCallsRdd, VariantsPca.scala:153-168).
 * Variant v's carriers are sample_idx[row_offsets[v] .. row_offsets[v+1]).  Host pointers.
 * Adds, for every variant and every ORDERED pair (c1, c2) of its carriers, 1 to S(c1, c2).
 * Replaces: the mapPartitions body of getSimilarityMatrix (VariantsPca.scala:184-189) and
 * sum_similarity (variants_pca.py:67-72).  Empty rows are legal (they add nothing; the reference
 * filters them at :166).  Repeated indices within a row count with multiplicity, as the
 * reference's double loop does (such a call runs on the int8 kernel; a call whose rows are sets --
 * everything a VCF yields -- goes to the MX-FP4 kernel; PCOA_FLAG_GRAM_FP4_MFMA turns a repeat into
 * PCOA_ERR_INVALID_ARG).  An index outside [0, N) -> PCOA_ERR_INDEX_RANGE, S unchanged by
 * that call's remaining chunks (reported at the next synchronising call at the latest). */
int pcoa_accumulate_calls(pcoa_ctx* ctx, const int32_t* sample_idx, const int64_t* row_offsets,
                          int64_t n_variants);

/* The same boundary with the caller saying where the arrays live (r04).  flags = 0 is pcoa_accumulate_calls: pageable host
 * arrays, consumed when the call returns.  What every form shares: the lists travel in chunks of <= 8 M entries through two
 * staging slots (H2D of chunk k+1 beside the scatter of chunk k), the DEVICE checks them (range, repeats), and a call is
 * only added to S once its check is clean -- PCOA_ERR_INDEX_RANGE leaves S as it was.
 *   PCOA_CALLS_HOST_PINNED  the arrays are page-locked (hipHostMalloc / hipHostRegister): the DMA engine reads them directly
 *                           (no copy into the library's pinned staging: ~10 GB/s per host thread against a 63 GB/s link).
 *   PCOA_CALLS_ASYNC        the arrays stay valid AND unmodified until the next synchronising call (pcoa_sync,
 *                           pcoa_gram_finalize, every read / compute / all-reduce / timing call): the call returns when
 *                           the work is queued; an error in its lists is reported by the call that next validates -- a later
 *                           accumulate call or that synchronising call -- and S is then unchanged by every call since the
 *                           last synchronising call that returned PCOA_OK.  A Spark host that builds batch k+1 while batch k
 *                           is on its way (VariantsPcaNative.scala) wants PINNED | ASYNC with two batch buffers.
 *   PCOA_CALLS_DEVICE_PTR   both arrays are device pointers (e.g. the output of a device-side VCF / BGEN decoder), read in
 *                           place; implies the lifetime rule of PCOA_CALLS_ASYNC, like every other device input.
 * Replaces: the same mapPartitions body (VariantsPca.scala:184-189); the partition iterator of :184 is what makes the
 * reference's boundary a stream of batches. */
#define PCOA_CALLS_DEVICE_PTR 1u
#define PCOA_CALLS_HOST_PINNED 2u
#define PCOA_CALLS_ASYNC 4u
int pcoa_accumulate_calls_ex(pcoa_ctx* ctx, const int32_t* sample_idx, const int64_t* row_offsets, int64_t n_variants,
                             uint32_t flags);

/* Dense boundary: a variants x samples tile, x[v*ld + i] = carrier multiplicity (0.0f / 1.0f for
 * well-formed input: extractCallInfo's hasVariation, VariantsPca.scala:56-60).  `x` is a host
 * pointer (is_device_ptr = 0; staged through pinned memory) or a device pointer (is_device_ptr = 1;
 * read in place, must stay valid until the next synchronising call).  ld >= N.
 * Replaces: the same mapPartitions body, with the RDD partition materialised as a matrix tile
 * (BASELINE.json configs[1]: "2,504 samples x 1M variants fp32").
 * Rates: a tile of 0 / 1 values runs the pipelined k-bits / MX-FP4 path.  A tile that holds carrier multiplicities
 * 2..127 (not produced by the reference's call extraction: hasVariation is a boolean) takes the int8 path, which is NOT
 * pipelined -- its pre-pass (one byte per genotype, 8x the operand bytes) and its contraction (int8 MFMA: half the MX-FP4
 * rate) run in series on the ctx stream -- at about half the rate of a binary tile (225 vs 480 M variants/s for fp32
 * tiles at N = 2504), and in the auto mode the tile is read twice (the binary pre-pass finds the multiplicity first).
 * Any ld >= N that keeps rows 16-byte aligned (ld % 4 == 0) takes the fast pre-pass; the pitch needs no padding to
 * 128-byte lines (measured: profiles/r04y_ring_pitch_sweep.txt). */
int pcoa_accumulate_dense_f32(pcoa_ctx* ctx, const float* x, int64_t n_variants, int64_t ld,
                              int is_device_ptr);

/* Same boundary with one byte per genotype (values 0..127): the production format -- a 4x cheaper re-layout pass than the
 * fp32 tile (SURVEY.md 8f "bit-packed / int8 Gram path").  Kernel choice as for the fp32 tile: in the default (auto) mode a
 * tile of 0 / 1 bytes goes to the MX-FP4 matrix cores (pcoa_timings.gram_kernel_kind == 3), a tile with carrier
 * multiplicities 2..127 to the int8 ones (== 2); the create flags force either.  Host or device pointer as above. */
int pcoa_accumulate_dense_u8(pcoa_ctx* ctx, const uint8_t* x, int64_t n_variants, int64_t ld, int is_device_ptr);

/* Bit-packed variants x samples tile: row v is the carrier BITSET of variant v, 1 bit per genotype; sample i is
 * bit (i & 31) of the little-endian word bits[v * ld_words + (i >> 5)], ld_words >= ceil(N / 32); bits of samples
 * >= N are ignored.  313 B per variant at N = 2504 (32x less than the fp32 tile: BASELINE configs[2]'s 40 M variants
 * are 12.5 GB).  Host or device pointer.  A bitset cannot repeat a callset, so the tile is binary by construction and
 * always runs on the MX-FP4 kernel (not available with PCOA_FLAG_GRAM_F32_MFMA).
 * Replaces: the same RDD[Seq[Int]] rows as pcoa_accumulate_calls (getCallsRdd, VariantsPca.scala:153-168; the
 * hasVariation indicator of extractCallInfo, :56-60), one bit per (variant, callset) instead of a list of indices;
 * SURVEY 8(d) "1-bit-packed twin", 8(f) rank 2. */
int pcoa_accumulate_bits(pcoa_ctx* ctx, const uint32_t* bits, int64_t n_variants, int64_t ld_words,
                         int is_device_ptr);

/* PLINK 1 binary genotypes as they lie in a variant-major .bed file (r04): bed_rows[v * row_bytes + s / 4] holds sample s of
 * variant v in bits 2 (s % 4): 00 homozygous A1, 01 missing, 10 heterozygous, 11 homozygous A2; row_bytes >= ceil(N / 4) (the
 * file's own pitch is exactly that; the three magic bytes are the caller's to skip).  A sample is a carrier of the variant --
 * hasVariation, VariantsPca.scala:56-60 -- iff its code is 10 or the homozygous NON-reference one: 00 when A2 is the reference
 * allele (plink --keep-allele-order / plink2 --make-bed; ref_is_a1 = 0), 11 when A1 is (ref_is_a1 = 1); a missing call
 * carries nothing.  The decode runs on the device (a host only reads the file: 626 B per variant at N = 2504), then the
 * bitset path of pcoa_accumulate_bits.  is_device_ptr: 0 host rows (consumed when the call returns), 1 device rows (lifetime
 * rule of every device input), PCOA_BED_HOST_ASYNC (r05) host rows in PAGE-LOCKED memory (pcoa_host_alloc_pinned) that the
 * call only QUEUES: it returns while the copy may still be running, so a host that rotates a few blocks keeps the link busy
 * while it reads the next block.  The rows of such a call must stay unmodified until the SECOND later call of this
 * function (with n_variants > 0) on the same ctx has returned (host rows travel through two device slots: a call that takes a slot first waits
 * for the decode of the call that used it last) or until any synchronising call (pcoa_sync, pcoa_gram_finalize, ..).
 * Replaces: the same RDD[Seq[Int]] rows (getCallsRdd, VariantsPca.scala:153-168) for a cohort stored as a PLINK fileset. */
#define PCOA_BED_HOST_ASYNC 2
int pcoa_accumulate_plink_bed(pcoa_ctx* ctx, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes, int ref_is_a1,
                              int is_device_ptr);

/* Generates variants [first_variant, first_variant + n_variants) of the synthetic model directly
 * in HBM and accumulates them (no host tile).  params->thresholds covers exactly that range.
 * r06: on the default engine the genotypes are written straight into the 1-bit operand (no fp32 staging tile, no pre-pass,
 * no host synchronisation per chunk); the call returns when the thresholds have been copied, the rest is queued. */
int pcoa_accumulate_synthetic(pcoa_ctx* ctx, const pcoa_synth_params* params, int64_t first_variant,
                              int64_t n_variants);

/* Fills a caller-owned DEVICE buffer x_dev[n_variants][ld] with the synthetic genotypes (0.0f/1.0f)
 * without accumulating -- used by bench.py to make the input resident before the timed region. */
int pcoa_synth_fill_f32(pcoa_ctx* ctx, const pcoa_synth_params* params, int64_t first_variant,
                        int64_t n_variants, float* x_dev, int64_t ld);

/* Completes the local accumulation: contracts what the accumulate calls have only packed so far (binary tiles
 * are re-laid out into a packed operand buffer (1 bit per genotype by default) when they arrive and contracted when the
 * buffer is full: 2^20 variants where two buffers alternate, never more than 2^22,
 * or here -- every reader of S below does the same), mirrors the computed triangle, folds int32 partials.
 * After it the full symmetric S of THIS ctx is readable.  Accumulation may continue afterwards
 * (S is additive: a natural checkpoint/resume point).  Inputs of the accumulate calls are consumed by their
 * pre-pass: a device pointer has to stay valid until the next synchronising call, not until the contraction.
 * Replaces (single GPU): reduceByKey(_ + _) (VariantsPca.scala:190). */
int pcoa_gram_finalize(pcoa_ctx* ctx);

/* Cross-GPU sum of the finalized S over all ranks of an RCCL communicator (ncclComm_t passed as
 * void*), in place on every rank, on the ctx stream.  One rank per GPU / per process.
 * Replaces (multi GPU): reduceByKey(_ + _, numReducePartitions) (VariantsPca.scala:190). */
int pcoa_gram_allreduce_rccl(pcoa_ctx* ctx, void* nccl_comm);

/* RCCL bootstrap helpers for hosts without their own (e.g. the Scala/JNI host): rank 0 obtains a
 * 128-byte unique id, ships it to the other ranks by its own means (Spark broadcast), then every
 * rank calls pcoa_comm_init.  *comm_out is an ncclComm_t. */
int pcoa_comm_unique_id(uint8_t out_id[128]);
/* Which RCCL the three calls above and pcoa_gram_allreduce_rccl are bound to.  libpcoa_hip.so does not link librccl: at
 * the first communicator call it binds the RCCL image the process has already mapped (a PyTorch process carries its own,
 * torch/lib/librccl.so -- one collective runtime per process, not two), else librccl.so.1 from the library's RUNPATH
 * (/opt/rocm/lib: the Scala / JNI host's case).  path_out receives the image's path, *version_out ncclGetVersion's code;
 * either may be NULL.  PCOA_ERR_RCCL if no RCCL can be found. */
int pcoa_comm_runtime(char* path_out, int32_t path_cap, int32_t* version_out);
int pcoa_comm_init(pcoa_ctx* ctx, const uint8_t id[128], int32_t rank, int32_t n_ranks,
                   void** comm_out);
int pcoa_comm_destroy(void* nccl_comm);
/* Number of ranks of a communicator (ncclCommCount) -- what a bench line or a host log prints to show that the collective
 * really spans the GPUs it was launched on.  *count_out = ranks. */
int pcoa_comm_count(void* nccl_comm, int32_t* count_out);

/* Page-locked host memory for input blocks a host fills and hands to the accumulate calls (hipHostMalloc): the DMA engine
 * reads it at link speed, pageable memory goes through the runtime's staging copy at a third of that.  Process-wide, not tied
 * to a ctx; at least one ctx (i.e. a HIP device) must exist.  (A JVM host passes such a block as a direct ByteBuffer.) */
int pcoa_host_alloc_pinned(size_t bytes, void** out);
int pcoa_host_free_pinned(void* p);

/* dst.S += src.S for two engines of the SAME process (r04): what a host with one ctx per GPU -- k host threads, no
 * collective runtime -- calls after the accumulation (host/variants_pca_driver --gpus k; a Spark executor with several GPUs).
 * Both ctxs are synchronised; src's total crosses by hipMemcpyPeerAsync (xGMI on a node; the ctxs may also share a device).
 * r06: when neither engine has an int64 part and the summed variant weights stay below 2^31 (the test pcoa_gram_allreduce_rccl
 * applies) the int32 matrices are added in place -- 4 N^2 bytes cross, nothing is widened, and the large-N upper-triangle
 * forms of computePca stay available on dst; otherwise src's total leaves as int64 and is added into dst's int64 matrix.
 * src is unchanged.  Integer sums: order and grouping of the reductions do not matter.
 * Replaces: reduceByKey(_ + _, conf.numReducePartitions()) (VariantsPca.scala:190, GenomicsConf.scala:42-45) inside one JVM. */
int pcoa_gram_reduce_from(pcoa_ctx* dst, pcoa_ctx* src);

/* S of every engine := the sum over the k engines of their finalized S: the reduction of ALL engines of one process at once
 * (called from one host thread after the feeding threads have joined), as a reduce-scatter and an all-gather over the engines'
 * own matrices.  The flat element range [0, N^2) of S is cut into k chunks of whole 16-byte quads -- with Q = ceil(N^2 / 4),
 * owner g takes the quads [g Q / k, (g + 1) Q / k); the last owner's chunk ends with the N^2 % 4 tail elements; a chunk is empty
 * when Q < k leaves it none.  Phase 1: owner g's kernel, on its own stream, reads chunk g of all k matrices and writes the sums
 * into its OWN matrix.  Phase 2: every engine copies chunk h from owner h behind that kernel's event.  Every link carries 1 / k
 * of the matrix at a time, every engine takes part, and nothing is staged: no exchange buffer of any size beside S (the chain
 * of pcoa_gram_reduce_from calls sends k - 1 whole matrices into engine 0, one after the other, through an N^2 staging buffer).
 *   root_only == 0: on return every engine holds the total (what pcoa_gram_allreduce_rccl leaves behind).
 *   root_only != 0: ctxs[0] holds the total; every other engine comes back as after pcoa_reset -- S zero, no int64 part, the
 *                   bound of the int32 entries zero, usable -- and, beyond what pcoa_reset does, with gram_variants = 0: its
 *                   variants are counted on ctxs[0] from now on (the sum over the engines), so they are not counted twice.
 *   k == 1: pcoa_gram_finalize.
 *   The sums are integers: the result is, entry for entry, what the pcoa_gram_reduce_from chain gives.  When no engine has an
 *   int64 part and the summed variant weights stay below 2^31 - 1 the int32 matrices are summed in place
 *   (pcoa_timings.reduce_int32_calls counts it on every engine that holds the total); otherwise every engine gets an int64 matrix
 *   for the totals (PCOA_ERR_OUT_OF_MEMORY before any kernel leaves the engines unchanged) and each total is narrowed back into
 *   the int32 matrix where it fits, as after every int64 import.
 * Refusals, all before any device work; afterwards every engine is as it was and still computes:
 *   PCOA_ERR_INVALID_ARG  ctxs NULL, k < 1, k > PCOA_REDUCE_MAX_ENGINES, a NULL entry, the same ctx twice, differing N
 *   PCOA_ERR_STATE        a strip owner or an operator ctx among them (the message names the kind and the index); engines on
 *                         different devices without mutual peer access (the message names the two devices): phase 1 reads the
 *                         peers' matrices from a kernel, and there is no staged fallback in this call -- reduce such engines with
 *                         pcoa_gram_reduce_from.
 * Every engine is then finalized and its input checks are read; a failure on engine g comes back with its code, the message on
 * ctxs[0] prefixed with the index.  A HIP failure once phase 1 has started leaves EVERY S undefined: the engines must be reset
 * (pcoa_reset) before they are used again.  Errors are reported on ctxs[0] (on pcoa_last_error(NULL) where that is no ctx).
 * Synchronising on every engine.
 * Replaces: reduceByKey(_ + _) (VariantsPca.scala:190) for the k engines of one JVM. */
#define PCOA_REDUCE_MAX_ENGINES 16
int pcoa_gram_reduce_peers(pcoa_ctx* const* ctxs, int32_t k, int32_t root_only);

/* What pcoa_gram_reduce_peers did on THIS engine, cumulative since pcoa_create / pcoa_reset_timings.  (A struct of its own:
 * the layout and the size of pcoa_timings are held fixed by its readers.)  It grows at its end; out_size = sizeof of the
 * struct the caller compiled against.  Synchronising, like pcoa_get_timings. */
typedef struct pcoa_reduce_peers_stats {
  int64_t reduce_peers_calls;     /* calls this engine took part in                                                       */
  double reduce_peers_seconds;    /* HIP-event time of this engine's chunk kernel plus its gather copies                  */
  int64_t reduce_peers_bytes_in;  /* bytes this engine read (phase 1) or copied (phase 2) from OTHER engines' matrices    */
} pcoa_reduce_peers_stats;
int pcoa_get_reduce_peers_stats(pcoa_ctx* ctx, pcoa_reduce_peers_stats* out, size_t out_size);

/* Host-driven reduction alternative (bench.py uses torch.distributed, whose "nccl" backend is RCCL):
 * export copies the finalized S as int64 [N][N] into a DEVICE buffer; import replaces S with the
 * (reduced) contents of a DEVICE buffer. */
int pcoa_gram_export_device_i64(pcoa_ctx* ctx, int64_t* dst_dev);
int pcoa_gram_import_device_i64(pcoa_ctx* ctx, const int64_t* src_dev);

/* Copies the finalized S to host as int64 [N][N] (all N^2 entries, zeros included, as
 * matrix.iterator emits them, VariantsPca.scala:189).  For parity tests and checkpoints. */
int pcoa_gram_read_i64(pcoa_ctx* ctx, int64_t* out_nxn);

/* Copies the block S[row0 .. row0+rows) x [col0 .. col0+cols) of the finalized S to host (row-major,
 * rows x cols int64).  For spot checks and sliced checkpoints when N^2 entries are too many to move. */
int pcoa_gram_read_block_i64(pcoa_ctx* ctx, int32_t row0, int32_t col0, int32_t rows, int32_t cols, int64_t* out);

/* Loads S from host int64 [N][N] (resume from a checkpoint, or enter at computePca with matrix
 * entries produced elsewhere: computePca(matrixEntries), VariantsPca.scala:198). */
int pcoa_gram_load_i64(pcoa_ctx* ctx, const int64_t* in_nxn);

/* ---- computePca ------------------------------------------------------------------------------ */

/* Runs row sums + double-centring only and copies B (fp64 [N][N]) and the row sums to host.
 * Either output may be NULL.  Replaces: computePca lines VariantsPca.scala:206-223
 * (center_matrix, variants_pca.py:84-121).  For parity tests of that stage. */
int pcoa_center_read_f64(pcoa_ctx* ctx, double* out_b_nxn, double* out_row_sums, int32_t* out_nonzero_rows,
                         double* out_matrix_mean);

/* computePca (VariantsPca.scala:198-231; perform_pca variants_pca.py:123-152) on the finalized S:
 * centring, then the num_pc principal components of B.
 *   out_components : N x num_pc COLUMN-major, i.e. the layout of pca.toArray (VariantsPca.scala:227):
 *                    component c of sample i is out_components[i + c*N]; unit 2-norm columns;
 *                    sign-normalised (largest-magnitude entry positive, ties -> lowest index)
 *                    unless PCOA_FLAG_NO_SIGN_NORM.
 *   out_eigenvalues: num_pc eigenvalues of B, ordered by decreasing magnitude -- the order of the
 *                    singular values of Cov that MLlib's SVD sorts by (s = lambda^2/(N-1)). May be NULL.
 *   out_nonzero_rows: rowSums.filter(_ > 0).size (VariantsPca.scala:207). May be NULL.
 * 0 < num_pc <= N, else PCOA_ERR_INVALID_ARG (MLlib: require(k > 0 && k <= n)).
 * Solver: Lanczos on the centred matrix (never materialised), a pair returned only after its TRUE residual
 * ||B u - theta u|| passed on the device; if the single-vector iteration does not verify (clustered leading eigenvalues,
 * slow spectra) the band iteration with thick restarts takes over (r06), then -- up to N = 16,384 -- the dense Householder
 * solver.  PCOA_ERR_NOT_CONVERGED is what is left when all of them fail (pcoa_timings.eig_method / lanczos_block_steps
 * tell which one answered). */
int pcoa_compute(pcoa_ctx* ctx, int32_t num_pc, double* out_components, double* out_eigenvalues,
                 int32_t* out_nonzero_rows);

/* Out-of-sample projection: places samples that took no part in the PCA onto a reference cohort's principal coordinates
 * (the Nystrom / Gower extension of computePca's output).  The reference's coordinate of sample i is row i of pca.toArray
 * (VariantsPca.scala:224-230): entry u_c[i] of a unit eigenvector of the double-centred B, and B u_c = lambda_c u_c gives
 * u_c[i] = (sum_j B(i, j) u_c[j]) / lambda_c.  A sample q to place gets its centred similarity row in place of B(i, .):
 *   x(j, q) = S(j, q) of cross (variants where reference sample j and q both carry), j in [0, ref->n)
 *   m_q     = (sum_j x(j, q)) / N_ref          (exact integer sum, one division: rowSums / rowCount, :206-215)
 *   b(q, j) = ((x(j, q) - m_q) - mean_j) + mm  (mean_j = rowSums_ref(j) / N_ref and mm = matrixMean of ref: the values
 *                                               pcoa_compute used on ref, bit for bit; the operation order of :216-221)
 *   coord(q, c) = (sum_j b(q, j) u_c[j]) / lambda_c   (j in fixed band order: deterministic, no floating-point atomics)
 * A reference sample projected this way lands on u_c[i] + r_c[i] / lambda_c, r_c = B u_c - lambda_c u_c the residual the
 * eigensolver verified before returning the pair.
 *   ref:   a full engine (pcoa_create) whose finalized S is the reference Gram.
 *   cross: a strip owner (pcoa_create_strip) with cross->n >= ref->n, fed the same variants: its rows [0, ref->n) are ref's
 *          samples in ref's order, its columns the samples to place (new ones, or reference ones).  It may sit on another
 *          device (the N_ref-double means travel by peer copy).
 *   components / eigenvalues: what pcoa_compute(ref, num_pc, ..) returned (host arrays, the same layout: [num_pc][ref->n]).
 *   out_coords: [num_pc][cols] column-major, the layout of out_components: component c of column q at out_coords[q + c*cols].
 * The pass reads rows [0, ref->n) of the strip once for the column sums and once per chunk of up to 8 components (num_pc = 2:
 * once).  PCOA_ERR_INVALID_ARG for a NULL pointer, num_pc outside (0, ref->n], cross->n < ref->n, ref a strip owner, cross not
 * one, or an eigenvalue that is zero or not finite; PCOA_ERR_STATE when an engine cannot serve (an input check of its
 * accumulation failed).  Errors are reported on ref.  Synchronising; neither S is modified.
 * Extends: computePca's output (VariantsPca.scala:224-246) to samples outside the matrix it decomposed. */
int pcoa_project(pcoa_ctx* ref, pcoa_ctx* cross, int32_t num_pc, const double* components, const double* eigenvalues,
                 double* out_coords);

/* ---- instrumentation ------------------------------------------------------------------------- */

/* Synchronises and fills *out.  Replaces: reportIoStats' role of printing what was processed
 * (VariantsPca.scala:48,281). */
int pcoa_get_timings(pcoa_ctx* ctx, pcoa_timings* out);
/* The struct grows at its end from release to release: pcoa_get_timings writes the r03 layout (PCOA_TIMINGS_R03_BYTES) and
 * nothing behind it; pass sizeof(pcoa_timings) of the header you compiled against here to receive the newer fields too. */
int pcoa_get_timings_sized(pcoa_ctx* ctx, pcoa_timings* out, size_t out_size);
int pcoa_reset_timings(pcoa_ctx* ctx);

/* ---- test hooks (not part of the reference-facing boundary) ---------------------------------------------------------------
 * Device memory from the library's own allocator.  With the environment variable PCOA_DEBUG_GUARD=1 (=2) every device
 * buffer of the library -- and these -- is a virtual range of its own whose END (START) lies against a page that is
 * never mapped: a kernel that reads or writes one element too far faults at once ("Memory access fault by GPU") instead
 * of touching a neighbouring allocation.  The GPU test suite runs its fuzz and parity sweeps in that mode with the
 * input tiles allocated here (tests/test_gpu_guard.py).  pcoa_debug_guard_mode returns the mode in effect (0 = off). */
int pcoa_debug_alloc(int32_t device_ordinal, size_t bytes, void** out);
/* One y = B x of the centred matrix of the current S (host vectors of N doubles) with one form of the eigensolver's mat-vec
 * (the numbers of pcoa_timings.matvec_form):
 * 0 = one wave per row over all N^2 entries of S, centred on the fly, 1 = upper-triangular 1024 x 1024 tiles, each entry read
 * once and used for y_i and y_j (the form pcoa_compute takes from N = 16,384; needs N % 4 == 0 and no int64 part, else
 * PCOA_ERR_STATE), 2 = one wave per row over the materialised B (the form of PCOA_EXPLICIT_CENTER; allocates the N x N fp64
 * matrix).  Any other form: PCOA_ERR_INVALID_ARG. */
int pcoa_debug_centred_matvec(pcoa_ctx* ctx, const double* x, double* y, int form);
/* The partition pcoa_gram_reduce_peers cuts S by: chunk g of k over N samples as [*first_out, *first_out + *count_out) of the flat
 * element range [0, N^2).  Pure function (no GPU): the one the library's launches and copies go by. */
int pcoa_debug_reduce_chunk(int32_t g, int32_t k, int32_t n_samples, int64_t* first_out, int64_t* count_out);
int pcoa_debug_free(void* p);
int pcoa_debug_guard_mode(void);

/* ---- environment knobs ---------------------------------------------------------------------------------------------------
 * For tests and measurements, not for users: nothing here is needed to use the library, and none is a stable interface.
 * Each selects a path or a threshold that a test, bench.py or a tool under tools/ runs on purpose.  All of them are read
 * once, at first use, in one place (debug_knobs(), csrc/devmem.hip).  One line per knob:
 *   PCOA_GRAM_KERNEL            auto | fp4 | i8 | f32: the Gram kernel, overriding the create flags
 *   PCOA_DEBUG_PACK_CHUNK       variants per pre-pass launch (forces the multi-chunk paths at test sizes)
 *   PCOA_DEBUG_MAX_LAUNCH       variants per contraction launch (forces the multi-launch / two-buffer paths)
 *   PCOA_DEBUG_FOLD_THRESHOLD   variants an int32 partial may hold before it is folded into int64
 *   PCOA_DEBUG_GUARD            1 | 2: every device buffer ends | starts at an unmapped page (see the test hooks above)
 *   PCOA_PIPELINE               0 | 1: the two-stream fp32 pipeline off | on wherever it fits
 *   PCOA_BITS_PIPELINE          1: bitset tiles through the co-resident pipeline instead of transpose and contraction in series
 *   PCOA_GRAM_LOCKSTEP          0 | 1: the lock-step contraction launch off | on wherever it fits
 *   PCOA_EXPLICIT_CENTER        set: the Lanczos path materialises the centred matrix B
 *   PCOA_SYMV_SYM_MIN_N         smallest N whose Lanczos mat-vec reads only the upper triangle of S (default 16,384)
 *   PCOA_LANCZOS_BAND           0: no band-Lanczos fallback; 2: only the band iteration
 *   PCOA_LANCZOS_BAND_MMAX      basis size of the band iteration (forces thick restarts)
 *   PCOA_SYNTH_TILE             1: pcoa_accumulate_synthetic through the fp32 staging tile and the pre-pass
 *   PCOA_NO_NARROW              1: an int64 S that fits int32 stays int64
 *   PCOA_OPERATOR_SEGMENT_ROWS  rows per segment of an operator ctx's bit store (crosses segment boundaries with a few hundred rows)
 *   PCOA_GRM_SEGMENT_ROWS       the same for a GRM ctx's genotype store
 *   PCOA_KBITS_MODE             0 | 2 | 4 | 5: launch form of the k-bits contraction (split-K, lock-step, even split, even split
 *                               per XCD k-segment)
 *   PCOA_KBITS_W4               0 | 1: the one-wave-per-SIMD k-bits contraction never | wherever it has its CUs to itself (default)
 *   PCOA_KBITS_W4_DIAG          0: one wave of a diagonal tile idles; 1..16: wave roles, cost of a diagonal stage in the even split
 *   PCOA_KBITS_CORESIDE         0 | 1: fp32 pipeline with pre-pass and contraction on disjoint | the same CUs
 *   PCOA_CSR_LEGACY             1: pcoa_accumulate_calls through the host-validated path
 */

/* Name of the GPU the ctx runs on, its CU count and the library version string. */
int pcoa_device_info(pcoa_ctx* ctx, char* name_out, int32_t name_cap, int32_t* cu_count_out);
const char* pcoa_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PCOA_H_ */
