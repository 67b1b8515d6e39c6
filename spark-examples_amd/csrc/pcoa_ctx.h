// pcoa_ctx.h -- what the translation units of the C ABI share (private, not installed): the engine's state (pcoa_ctx),
// error reporting, HIP-event timing, and the helpers that cross files.  Host-side orchestration only: device memory
// ownership, chunking (fp32 accumulators stay exact below 2^24 per launch, int32 partials are folded into int64 before 2^31),
// stream ordering.  Who defines what:
//   devmem.hip           the allocator (guard pages), regrow, debug_knobs
//   operand.hip          S and its int64 fold, the operand buffers, the contractions, finalize
//   row_feed.hip         the staging ring; row_feed.h beside it: the loop that brings bitset / .bed rows through the ring
//   capi_accumulate.hip  the input boundaries
//   capi_reduce.hip      RCCL, reductions, export / import / read / load
//   reduce_peers.hip     the partition and the chunk kernel of pcoa_gram_reduce_peers
//   capi_compute.hip     the eigensolver workspace, computePca, strips, projection
//   capi_operator.hip    the implicit similarity operator: the bit store, its products, computePca over it
//   capi_grm.hip         the standardised-genotype operator (pcoa_create_grm): the 2-bit store, its counts and weights, K x
//   capi_grm_project.hip SNP weights of K's axes and the projection of a study store onto them (pcoa_create_grm_study, pcoa_grm_weights / _project)
//   capi_grm_lsq.hip     pcoa_grm_project_lsq: the least-squares projection of sparsely called study samples (normal equations per sample)
//   capi_grm_dense.hip   pcoa_grm_block: a rectangle of K and of the pair counts read out through the fp64 matrix cores
//   capi_grm_ld.hip      pcoa_grm_ld_*: LD pruning of the resident GRM store by dosage r^2, as a keep mask that enters used_v
//   capi_grm_king.hip    pcoa_grm_king_block / pcoa_grm_king_pairs: the KING-robust kinship screen on the resident 2-bit store
//   capi_grm_pcrelate.hip pcoa_pcrelate_hat, pcoa_grm_pcrelate_*: PC-Relate kinship from a fit of the dosages on the axes, resident on the ctx
//   capi_grm_qc.hip      pcoa_grm_set_variant_filters, pcoa_grm_hwe, pcoa_grm_sample_counts: variant and sample QC on the resident store
//   capi_grm_subset.hip  pcoa_create_grm_subset: a new GRM ctx over a sample subset of another's store; pcoa_grm_rows reads rows back
//   capi_subset.hip      pcoa_create_subset: a new engine whose S is S[I, I] of another
//   capi_pairs.hip       pcoa_similar_pairs: the screen of S for duplicate and related sample pairs
//   capi_measure.hip     pcoa_set_similarity / pcoa_get_similarity and the centring of a Jaccard / cosine measure
//   capi_loadings.hip    pcoa_loadings_*: per-variant loadings of the principal coordinates from bitsets, .bed rows, the store
//   capi_ld.hip          pcoa_ld_*: LD pruning of the variant rows in front of the accumulation
//   capi_complete.hip    pcoa_set_call_companion / pcoa_accumulate_plink_bed_calls: the pairwise-complete similarity
//   capi_king.hip        pcoa_accumulate_plink_bed_king / pcoa_king_pairs: the KING-robust kinship screen over five planes
//   pcoa_capi.hip        create / destroy, errors, timings
#pragma once

#include <algorithm>
#include <chrono>

#include "pcoa_internal.h"

enum TimeCat { T_GRAM = 0, T_DENSIFY, T_SYNTH, T_FINALIZE, T_CENTER, T_TRIDIAG, T_EIG, T_BACK, T_PACK, T_LANCZOS, T_ALLREDUCE, T_OPERATOR, T_SUBSET, T_REDUCE_PEERS, T_PAIRS, T_LOADINGS, T_LD_COUNT, T_LD_BAND, T_LD_RESOLVE, T_LD_COMPACT, T_KING, T_GRM_BLOCK, T_GRM_LD_BAND, T_GRM_LD_RESOLVE, T_GRM_LD_SCAN, T_GRM_SUBSET, T_GRM_PAIRS_DENSE, T_GRM_PAIRS_SCREEN, T_GRM_QC_HWE, T_GRM_QC_SAMPLES, T_GRM_LSQ_PAIRS, T_GRM_LSQ_SOLVE, T_GRM_KING_COUNTS, T_GRM_KING_SCREEN, T_GRM_PCR_FIT, T_GRM_PCR_DENSE, T_GRM_PCR_SCREEN, T_NCAT };

struct EventPair {
  hipEvent_t a, b;
  int cat;
};

// A ring of two staging slots: the double-buffered host-to-device staging of a host caller's input on the copy stream
// (pcoa_ctx::csr_stream), so that the copy of one chunk runs beside the kernels of the chunk before.  The protocol, in the
// order a boundary goes through it (row_feed.hip; the bitset and .bed boundaries go through it in row_feed.h):
//   staging_acquire    the next slot; the host waits for the slot's last reader (`freed`) before the slot may be rewritten
//                      or regrown -- sizes are the boundary's own policy: it names what it needs and what to grow to
//   (the copies, on the copy stream)
//   staging_copied     `copied` recorded behind them; the boundary makes its consumer stream wait for it, and a synchronous
//                      call ends with the host waiting for the last `copied`: a host input is consumed when its copy is
//                      done, not when its kernels are
//   staging_released   `freed` recorded behind the slot's last reader, on the stream the boundary names
// A slot has two device buffers under one event pair (the carrier lists travel as indices + offsets; the other rings use
// buffer 0 only), each with an optional page-locked twin for pageable sources (staging_pin).
struct StagingRing {
  struct Slot {
    void* dev[2] = {nullptr, nullptr};
    size_t dev_bytes[2] = {0, 0};
    void* pin[2] = {nullptr, nullptr};
    size_t pin_bytes[2] = {0, 0};
    hipEvent_t copied = nullptr, freed = nullptr;   // H2D of the slot done / the kernels that read the slot done
    bool used = false;
  };
  Slot slot[2];
  int next = 0;   // slot[next & 1] is acquired next
};

struct pcoa_ctx {
  int32_t n = 0;
  // strip owner (SURVEY 8e, N beyond one HBM): the ctx holds S[:, strip_col0 .. strip_col0 + s_cols) as [n][s_cols]
  // (both triangles, no mirror); s_cols == n and is_strip == false for the ordinary symmetric engine
  int32_t s_cols = 0, strip_col0 = 0;
  bool is_strip = false;
  double* strip_ws = nullptr;      // partial sums of the strip reductions (lazy)
  int64_t strip_ws_cap = 0;
  double* strip_means = nullptr;   // [n] rowSums / N, resident between the mat-vecs of one computePca (pcoa_strip_set_centering)
  double strip_matrix_mean = 0.0;
  bool strip_centering_set = false;
  double* proj_ws = nullptr;       // pcoa_project on a strip owner: reference means, components, eigenvalues, partials, result (lazy)
  int64_t proj_ws_cap = 0;
  // implicit similarity operator (pcoa_create_operator, capi_operator.hip): the ctx holds the carrier bitsets of every variant
  // it was fed, in segments of op_seg_rows rows that are never reallocated or copied, and no N x N matrix of any kind
  bool is_operator = false;
  struct OpSegment { uint32_t* p; int64_t rows; };
  std::vector<OpSegment> op_segs;
  int64_t op_seg_rows = 0;         // rows a segment holds
  int64_t op_variants = 0;         // rows in the store
  bool op_centering_set = false;   // row_sums / stats / colmean / nz belong to the current store
  double* op_ws = nullptr;         // t, the passes' partials, the two dots (sized by the store, lazy)
  int64_t op_ws_cap = 0;
  int64_t op_products = 0;
  // standardised-genotype operator (pcoa_create_grm, capi_grm.hip): is_operator is set too -- the ctx keeps rows in the same
  // segmented store (op_segs .. op_ws, op_centering_set: the counts belong to the current store) and no N x N matrix -- but the
  // rows are 2-bit genotypes at grm_pitch_words(n) words and the product is K x, K = A^T diag(d) A / M'
  bool is_grm = false;
  double grm_min_maf = 0.0;        // pcoa_grm_set_min_maf; survives pcoa_reset
  bool grm_weights_set = false;    // mu / d / used / M' belong to the current counts and grm_min_maf
  int32_t* grm_cnt = nullptr;      // [V][3] called, het, hom non-reference, then [V] used (lazy, sized by the store)
  int64_t grm_cnt_cap = 0;
  double* grm_par = nullptr;       // [V] mu, [V] d, then M' (one 64-bit count)
  int64_t grm_par_cap = 0;
  int64_t grm_used = 0;            // M' of the current weights
  bool is_grm_study = false;       // pcoa_create_grm_study: a GRM store of study samples with no weights of its own (capi_grm_project.hip)
  double* grm_mw = nullptr;        // pcoa_grm_weights / pcoa_grm_project on a panel: components, t, s, the passes' partials, results (lazy)
  int64_t grm_mw_cap = 0;
  double* grm_blk = nullptr;       // pcoa_grm_block: [rows][cols] doubles, then as many int32 where the pair counts are needed (lazy)
  int64_t grm_blk_cap = 0;
  int64_t grm_block_calls = 0;     // pcoa_grm_block_stats
  double grm_block_flops = 0;
  int64_t grm_pairs_calls = 0, grm_pairs_bands = 0, grm_pairs_bytes = 0;   // pcoa_grm_pairs_stats (the bands live in grm_blk)
  double grm_pairs_flops = 0;
  int64_t grm_king_calls = 0, grm_king_block_calls = 0, grm_king_bands = 0, grm_king_bytes = 0;   // pcoa_grm_king_stats (the bands live in grm_blk)
  double grm_king_macs = 0;
  // PC-Relate (capi_grm_pcrelate.hip): the fit is a statement about the store's rows and the two matrices of the fit call alone; an
  // append and pcoa_reset drop it (grm_pcr_drop), a subset does not inherit it
  double* grm_pcr = nullptr;       // beta [V][n_cov], then basis [n_cov][N] (sized by the fit)
  int64_t grm_pcr_cap = 0;
  bool grm_pcr_set = false;
  int32_t grm_pcr_cov = 0;         // n_cov of the resident fit
  int32_t grm_pcr_dropped_by = 0;  // what dropped the last fit: 0 nothing (never fitted), 1 an accumulate call, 2 pcoa_reset, 3 a failed fit
  int64_t grm_pcr_fits = 0, grm_pcr_block_calls = 0, grm_pcr_pairs_calls = 0, grm_pcr_bands = 0, grm_pcr_bytes = 0;   // pcoa_grm_pcrelate_stats
  double grm_pcr_flops = 0;
  // LD pruning of the store (pcoa_grm_ld_prune, capi_grm_ld.hip): the keep mask is a statement about the store as it was
  // pruned under grm_min_maf; an append, pcoa_reset, another min_maf and pcoa_grm_ld_clear drop it (grm_ld_drop)
  uint8_t* grm_keep = nullptr;     // [V] 1 = kept, 0 = removed or no candidate
  int64_t grm_keep_cap = 0;
  bool grm_keep_set = false;
  int64_t grm_ld_rows = 0, grm_ld_cand = 0, grm_ld_kept = 0, grm_ld_pairs = 0;   // the last prune, for pcoa_get_grm_ld_stats
  // variant and sample QC (capi_grm_qc.hip): the two filters are properties of the ctx like grm_min_maf -- they survive pcoa_reset,
  // a subset inherits them, another value marks the weights stale and drops the keep mask.  The p-values are resident beside the
  // counts (grm_hwe_set: they belong to the current counts) and computed only when hwe_min_p > 0 or pcoa_grm_hwe asks
  double grm_max_missing = 1.0, grm_hwe_min_p = 0.0;
  double* grm_hwe = nullptr;       // [V] (lazy)
  int64_t grm_hwe_cap = 0;
  bool grm_hwe_set = false;
  int32_t* grm_qc_part = nullptr;  // pcoa_grm_sample_counts: [ranges][3][pitch * 16] int32 partials (lazy)
  int64_t grm_qc_part_cap = 0;
  int64_t* grm_qc_out = nullptr;   // [N][3] results, then the three fail counts of pcoa_get_grm_qc_stats (lazy)
  int64_t grm_qc_out_cap = 0;
  int64_t grm_hwe_calls = 0, grm_sample_counts_calls = 0;
  int64_t grm_lsq_calls = 0, grm_lsq_pair_vectors = 0, grm_lsq_undetermined = 0;   // pcoa_get_grm_lsq_stats (capi_grm_lsq.hip; the work lives in grm_mw)
  int64_t grm_subset_calls = 0, grm_subset_bytes = 0;   // pcoa_create_grm_subset with this ctx as src (pcoa_get_grm_subset_stats)
  int64_t subset_bytes = 0;        // bytes the gathers of pcoa_create_subset moved into this ctx (read + written)
  int64_t pairs_bytes = 0, pairs_calls = 0;   // pcoa_similar_pairs: bytes of S its scan kernels read, calls
  // per-variant loadings (pcoa_loadings_begin .. pcoa_loadings_end, capi_loadings.hip): the prepared vectors stay resident
  // between begin and end; the decode and output buffers are kept until pcoa_destroy
  bool ld_active = false;
  int32_t ld_num_pc = 0;
  double* ld_u = nullptr;          // [num_pc][32 ceil(n / 32)] prepared vectors (centred where asked, zero for i >= n), then num_pc divisors
  int64_t ld_u_cap = 0;
  const double* ld_div = nullptr;  // sqrt(eigenvalues) behind the vectors (PCOA_LOADINGS_UNIT), else NULL
  uint32_t* ld_bits = nullptr;     // decoded .bed rows of one chunk (lazy)
  int64_t ld_bits_cap = 0;
  double* ld_out = nullptr;        // one chunk of results on their way to a host `out` (lazy)
  int64_t ld_out_cap = 0;
  int64_t ld_variants = 0, ld_bytes = 0;   // rows the loadings kernels took, bytes of bitsets they read
  // LD pruning (pcoa_ld_begin .. pcoa_ld_end, capi_ld.hip).  The work buffer holds the carried tail -- the last ldp_tail <=
  // ldp_window rows, at rows [ldp_window - ldp_tail, ldp_window) -- in front of the rows of one chunk; every buffer is sized by
  // pcoa_ld_begin and lives until pcoa_ld_end
  bool ldp_active = false, ldp_accumulate = false;
  int32_t ldp_window = 0, ldp_tail = 0;
  double ldp_r2 = 0.0;
  int64_t ldp_chunk = 0;           // rows of a chunk (the capacity behind the tail)
  int64_t ldp_pos = 0;             // rows fed since the last break
  uint32_t* ldp_wb = nullptr;      // [window + chunk][ceil(n / 32)] rows, tail bits cleared
  int32_t* ldp_cnt = nullptr;      // [window + chunk] carrier counts
  uint32_t* ldp_tmp = nullptr;     // [window] rows + [window] counts: the tail of a chunk shorter than the window on its way down
  uint32_t* ldp_ex = nullptr;      // [chunk][ceil(window / 32)] band words
  uint32_t* ldp_flags = nullptr;   // [64] keep flags of the resolve wave
  uint32_t* ldp_kbits = nullptr;   // [chunk / 32 + 2] the chunk's keep flags as the resolve wave holds them
  uint8_t* ldp_keep = nullptr;     // [chunk] the same as bytes
  int32_t* ldp_scan = nullptr;     // [chunk] place among the kept rows
  int64_t* ldp_out2 = nullptr;     // {kept, monomorphic} of a chunk
  uint32_t* ldp_compact = nullptr; // [chunk][ceil(n / 32)] kept rows (PCOA_LD_ACCUMULATE)
  uint32_t* ldp_bed = nullptr;     // decoded .bed rows of one chunk (lazy)
  int64_t ldp_bed_cap = 0;
  int64_t ldp_seen = 0, ldp_kept = 0, ldp_mono = 0, ldp_pairs = 0;
  int device = 0;
  uint32_t flags = 0;
  int num_cu = 256;
  char dev_name[256] = {0};
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string last_error;

  // Gram state
  int32_t* s32 = nullptr;          // [n][n] partial, upper-triangular tiles authoritative
  int64_t* s64 = nullptr;          // [n][n] folded total (lazy), always symmetric
  int64_t* s64_spare = nullptr;    // an int64 matrix retired by narrow_s64 (S fitted int32 again): the next fold re-uses it
  int64_t variants_in_s32 = 0;     // variants accumulated into s32 since the last fold
  bool dirty = false;              // s32 has contributions not yet mirrored
  float* zeros = nullptr;          // 4 KiB of zeros
  int32_t* err_flag = nullptr;     // device: [0] error bits, [1] max carrier multiplicity seen by the int8 pre-passes
  // Pinned host memory where every small asynchronous read-back of the library lands (flags, multiplicity bound,
  // statistics, the all-reduce's agreement words).  Never a stack variable or pageable memory: an async copy to
  // pageable memory goes through the runtime's staging path and its helper thread.
  struct HostWords {
    int32_t flag, mmax, seen, nz;
    int64_t coll[2];
    double st[2];
    int64_t ld[2];   // {kept, monomorphic} of an LD-pruning chunk
    int32_t cflag;   // complete_diag_kernel's flag: some Q(i, i) > V
    int32_t kflag[pcoa::kKingFlagWords];   // the four consistency checks of the kinship screen
    int64_t king[3]; // its V, n_found and the entries the write pass read again
    int64_t grm[2];  // M' of a GRM ctx's weights
    int64_t qc[3];   // the fail counts of pcoa_get_grm_qc_stats
    int32_t lsq;     // the undetermined samples of a pcoa_grm_project_lsq call
  };
  HostWords* hw = nullptr;

  // staging (lazy)
  float* tile = nullptr;
  int64_t tile_elems = 0;
  int32_t* csr_idx = nullptr;
  int64_t csr_idx_cap = 0;
  int64_t* csr_offs = nullptr;
  int64_t csr_offs_cap = 0;
  // CSR boundary, fast path (calls_fast): two staging slots (device idx / offsets + a pinned host twin for pageable
  // callers), a copy stream, a flag word of its own, and the chunks whose validation is still owed
  StagingRing cs;   // buffer 0: indices (int32), buffer 1: offsets (int64)
  hipStream_t csr_stream = nullptr;
  int32_t* csr_flag = nullptr;        // device: bit 0 index out of range, bit 5 a carrier list repeats a callset
  int32_t* csr_flag_host = nullptr;   // pinned
  struct CsrPending { const int32_t* idx; const int64_t* offs; int64_t nv; int64_t kb; bool device; };
  std::vector<CsrPending> csr_pending;  // committed provisionally into the ACTIVE operand buffer, not yet validated
  double csr_stage_s = 0, csr_wait_s = 0;  // host seconds spent copying into pinned staging / waiting in validation
  int64_t csr_fast_chunks = 0, csr_redo_chunks = 0;
  // raw PLINK .bed rows (pcoa_accumulate_plink_bed, host input): two device slots filled on the copy stream (csr_stream),
  // so that the H2D of one chunk runs beside the decode / transpose / contraction of the one before
  StagingRing bs;   // shared with the host bitsets of pcoa_accumulate_bits
  uint32_t* thr_dev = nullptr;
  int64_t thr_cap = 0;
  int32_t* sample_pop = nullptr;   // [n]
  std::vector<int32_t> pop_offsets_dev;   // the pop_offsets sample_pop was built from (uploaded again only when they change)
  // pcoa_accumulate_synthetic, k-bits operand (r06): the thresholds of a call travel on the copy stream into one of two slots
  StagingRing ts;
  int64_t* xfer = nullptr;         // exchange buffer (lazy): [n][n] int64, or [n][n] int32 for the int32 peer reduction
  size_t xfer_bytes = 0;
  int32_t* narrow_flag = nullptr;  // device: narrow_s64's {overflow, -, max |entry| (64 bit)}
  int64_t reduce_i32_calls = 0, narrowed = 0, allreduce_calls = 0;
  int64_t reduce_peers_calls = 0, reduce_peers_bytes_in = 0;   // pcoa_gram_reduce_peers: calls, bytes read or copied from OTHER engines
  int32_t comm_ranks = 0, allreduce_int32 = 0, matvec_form = 0, lanczos_block_steps = 0;
  int64_t* coll = nullptr;         // 2 int64: {variants in S32, has-S64 flag} agreed across ranks
  int8_t* pack_buf = nullptr;      // k-blocked int8 workspace of the i8 path (lazy)
  int64_t pack_cap = 0;            // bytes
  bool use_i8 = true;              // packed-operand Gram (FP4 / int8) or fp32-MFMA Gram
  int packed_mode = 0;             // 0 auto (FP4 for binary tiles, int8 otherwise), 2 int8 only, 3 FP4 only
  // Form of the binary-tile operand in HBM: 2 = k-bits (1 bit per genotype, expanded to MX-FP4 in registers by the
  // contraction: gram_kbits.hip; default), 1 = MX-FP4 (4 bits per genotype, PCOA_FLAG_OPERAND_FP4).  The buffer logic
  // below counts in k-blocks of 32 variants either way; a k-bits chunk is padded to whole blocks of 128 variants.
  int op_fmt = 2;
  int64_t fp4_fallbacks = 0;
  int i8_streak = 0;               // auto mode: chunks still to be sent straight to the int8 kernel after a fallback
  // FP4 operand buffers.  Binary chunks are only PACKED when they arrive (behind what the active buffer already
  // holds); a buffer is contracted when it is full or when S is needed (finalize / read / all-reduce / compute), so one
  // launch carries up to the buffer's capacity whatever the size of the calls.  Two buffers exist where the fp32
  // pipeline applies (fb_count == 2): the pre-pass of the next buffer then runs beside the contraction of the last one
  // on disjoint CU sets (DESIGN_HISTORY.md 4.1).  Auto mode: the pre-passes of a buffer generation raise the buffer's device
  // flag on a value other than 0 / 1, the contraction reads the same word and does nothing if it is set, and the host
  // learns it when it next needs the buffer (fp4_resolve) and redoes the generation's chunks on the int8 kernel -- no
  // host synchronisation per call.
  struct Fp4Chunk { const void* x; int is_u8; int64_t nv, ld; };
  struct Fp4Buf {
    int8_t* p = nullptr;
    int64_t cap_kb = 0;            // capacity in k-blocks of 32 variants (+24 of zero padding behind it)
    int64_t kb = 0, vars = 0;      // filled: k-blocks / variants (the last k-block of a chunk may be partly empty)
    hipStream_t fill_stream = nullptr;   // where this generation's pre-passes run (ctx stream or the masked pack stream)
    hipEvent_t packed = nullptr, consumed = nullptr;
    bool launched = false;         // the contraction of the last generation is queued; `consumed` tells when it is done
    bool verify = false;           // that generation's pre-passes report non-binary values through the buffer's flag
    int64_t launched_vars = 0;
    std::vector<Fp4Chunk> chunks;  // device-resident inputs of the generation (kept until it is verified)
  };
  Fp4Buf fb[2];
  int fb_count = 1, fb_active = 0;
  int32_t* fb_flags = nullptr;       // device: the flag word of buffer b at fb_flags[16 * b]
  int32_t* fb_flags_host = nullptr;  // pinned host copy, written by an async D2H behind each contraction
  // fp32 pipeline: the pre-pass of one buffer beside the lock-step contraction of the other, on two side streams
  bool pipe_ok = false;
  int pipe_gram_cus = 0;
  hipStream_t pack_stream = nullptr, gram_stream = nullptr;
  hipEvent_t ev_fork = nullptr;
  bool lockstep_ok = false;          // the lock-step contraction launch fits this N on the whole chip
  int kbits_mode = 4;                // whole-chip launch form of the k-bits contraction: 4 even split, 2 lock-step, 0 split-K
  bool coreside = false;             // fp32 pipeline, k-bits operand: ring pre-pass and whole-chip contraction share every CU
  int coreside_mode = 4;             // launch form of that contraction: 2 lock-step where the shape fits, else 4 even split
  int ring_wgs = 0;                  // workgroups of the ring pre-pass beside a contraction
  int64_t lockstep_launches = 0, pipeline_launches = 0, evensplit_launches = 0;
  int64_t pack_chunk = (int64_t)1 << 20;  // variants packed + contracted per launch pair
  int64_t pack_launches = 0;
  double pack_bytes = 0;

  // computePca workspace (lazy)
  bool ws_ready = false;
  pcoa::EigWorkspace ws{};
  double* row_sums = nullptr;      // [n]
  double* colmean = nullptr;       // [n] rowSums / N (implicit form of B for the Lanczos path)
  double* stats = nullptr;         // [2 + n] (sum, mean, then int64 row sums)
  int32_t* nz = nullptr;           // [1]
  double* out_dev = nullptr;       // [kmax][n]
  int32_t kmax = 0;
  double* lanczos_ws = nullptr;    // Krylov basis + scalars of the Lanczos fast path (lazy)
  double* sym_part = nullptr;      // tile sums of the symmetric mat-vec (large N, lazy)
  int64_t sym_part_cap = 0;
  int64_t lanczos_cap = 0;         // doubles
  int32_t eig_method = 0;          // of the last pcoa_compute: 1 = Lanczos, 2 = Householder
  int32_t eig_dense_form = 0;      // EIG_FORM_* bits of the last pcoa_compute's dense solve of B (0 unless eig_method == 2)
  int32_t lanczos_steps = 0;
  // pcoa_set_similarity: what computePca decomposes (PCOA_SIMILARITY_*).  A property of the ctx like its create flags: it
  // survives pcoa_reset and a subset inherits it.  Nothing of a centring is kept between calls (every pcoa_compute /
  // pcoa_center_read_f64 starts from the row sums), so a change has nothing to invalidate beyond these two buffers' contents,
  // which are rewritten from S by every centring.
  int32_t similarity = 0;
  int64_t* measure_diag = nullptr;   // [n] (lazy)
  double* measure_q = nullptr;       // [n] (lazy)
  // pcoa_set_call_companion (capi_complete.hip): the engine that holds Q, the Gram matrix of the missing-call bitsets, and V.
  // Like the measure a property of how the ctx decomposes: it survives pcoa_reset; a subset gets a companion of its own
  // (Q[keep, keep]), which it owns and destroys.
  pcoa_ctx* companion = nullptr;
  int64_t companion_v = 0;
  bool companion_owned = false;
  int64_t* complete_c = nullptr;     // [n] c_i = V - Q(i, i), then the diagonal kernel's flag word (lazy)
  // pcoa_accumulate_plink_bed_calls: the missing-call rows of one chunk (the carrier rows go to `tile`), and the two events
  // that order this ctx's stream and the companion's around that buffer
  uint32_t* calls_bits = nullptr;
  int64_t calls_bits_cap = 0;
  hipEvent_t calls_decoded = nullptr, calls_read = nullptr;
  bool calls_read_pending = false;   // the companion's pre-pass of the last chunk may still be reading calls_bits
  // pcoa_accumulate_plink_bed_king, on planes[0] (capi_king.hip): the five planes' rows of one chunk, [plane][rows][words]; the
  // event the planes 1 - 4 wait for behind the decode, and the event each of them records behind its pre-pass of the chunk
  uint32_t* king_bits = nullptr;
  int64_t king_bits_cap = 0;
  hipEvent_t king_decoded = nullptr, king_read[PCOA_KING_PLANES] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool king_read_pending = false;    // those pre-passes may still be reading king_bits
  int64_t king_bytes = 0, king_calls = 0;   // pcoa_king_pairs: bytes of the five matrices its scan kernels read, calls

  // timings
  std::vector<EventPair> pending;
  std::vector<hipEvent_t> pool;
  double tsec[T_NCAT] = {0};
  int64_t gram_launches = 0;
  int64_t gram_variants = 0;
  double gram_flops = 0, gram_bytes = 0;
  double compute_total = 0;
  int gram_kind = 1;
  int64_t max_launch = (int64_t)1 << 24;
  int64_t fold_threshold = (int64_t)1 << 30;
};

#define HIP_TRY(ctx, expr)                                     \
  do {                                                         \
    hipError_t _e = (expr);                                    \
    if (_e != hipSuccess) return hip_fail((ctx), _e, #expr);   \
  } while (0)

#define CHECK_CTX(ctx)                                                      \
  do {                                                                      \
    if (!(ctx)) return fail(nullptr, PCOA_ERR_INVALID_ARG, "ctx is NULL");  \
    hipError_t _e = hipSetDevice((ctx)->device);                            \
    if (_e != hipSuccess) return hip_fail((ctx), _e, "hipSetDevice");       \
  } while (0)

// the calls that read or move S do not exist on an operator ctx
#define NOT_ON_OPERATOR(ctx, what)                                                                                       \
  do {                                                                                                                   \
    NOT_ON_GRM(ctx, what);                                                                                               \
    if ((ctx)->is_operator)                                                                                              \
      return fail((ctx), PCOA_ERR_STATE, what ": an operator ctx (pcoa_create_operator) holds the carrier bitsets, not " \
                                         "S; use a full engine (pcoa_create) for this call");                         \
  } while (0)

// nor on a GRM ctx, which also has none of the calls that take or read carrier bitsets
#define NOT_ON_GRM(ctx, what)                                                                                              \
  do {                                                                                                                     \
    if ((ctx)->is_grm)                                                                                                     \
      return fail((ctx), PCOA_ERR_STATE, what ": a GRM ctx (pcoa_create_grm) holds 2-bit genotype rows fed through "       \
                                         "pcoa_accumulate_plink_bed, no S and no carrier bitsets; its calls are "         \
                                         "pcoa_grm_* and pcoa_compute");                                                  \
  } while (0)

namespace pcoa {

constexpr int64_t KB_I8 = 16;                             // variants per int8 k-block
constexpr int64_t kMaxLaunchVariants = (int64_t)1 << 24;  // fp32 accumulators exact below 2^24
constexpr int64_t kFoldThreshold = (int64_t)1 << 30;      // fold int32 partials long before 2^31
constexpr int64_t kBatchVariants = (int64_t)1 << 22;   // variants per FP4 contraction launch (fp32 exact below 2^24)
constexpr int64_t kBatchBytes = (int64_t)6 << 30;      // cap of an FP4 operand buffer
constexpr int64_t kPipeVariants = (int64_t)1 << 20;    // buffer size where two buffers alternate (pipeline / lock-step)
constexpr int64_t kCoresideMaxNpad = 16384;            // co-resident pipeline: largest padded sample count (measured up to here)

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline int64_t words_of(const pcoa_ctx* c) { return ((int64_t)c->n + 31) / 32; }   // words of a carrier bitset row
inline size_t s_count(const pcoa_ctx* c) { return (size_t)c->n * (size_t)c->s_cols; }
inline GramStrip strip_of(const pcoa_ctx* c) {
  GramStrip st;
  if (c->is_strip) { st.col0 = c->strip_col0; st.cols = c->s_cols; }
  return st;
}

// ---- devmem.hip: every device allocation of the library goes through dev_alloc / dev_free
hipError_t dev_alloc(void** out, size_t bytes, int device);
void dev_free(void* p);
int regrow(pcoa_ctx* c, void** buf, size_t bytes, bool sync_ctx_stream);
// kernels on `peer_device` may read and write the buffer p (a dev_alloc result on another device).  A plain allocation is
// covered by hipDeviceEnablePeerAccess (the caller's); a guard-page mapping needs its own hipMemSetAccess naming the peer
hipError_t dev_grant_peer(void* p, int owner_device, int peer_device);

// ---- pcoa_capi.hip: errors (c == nullptr: the thread's create error) and the timing events
int fail(pcoa_ctx* c, int code, const std::string& msg);
int hip_fail(pcoa_ctx* c, hipError_t e, const char* what);
int create_full_engine_unfilled(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags);   // pcoa_create, S not zeroed
int create_grm_engine(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags);             // pcoa_create_grm
int create_grm_study_engine(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags);       // pcoa_create_grm_study
hipEvent_t get_event(pcoa_ctx* c);
void drain_events(pcoa_ctx* c, bool wait);

// ---- operand.hip
int fold_now(pcoa_ctx* c);
int ensure_xfer(pcoa_ctx* c, size_t bytes);
int narrow_s64(pcoa_ctx* c);
int take_s64(pcoa_ctx* c);      // c->s64 := the spare, else a fresh allocation; contents undefined
void retire_s64(pcoa_ctx* c);   // c->s64 becomes the spare (small N) or is freed; c->s64 = nullptr
void account_gram(pcoa_ctx* c, int64_t cur, int64_t weight = 1);
int fold_if_needed(pcoa_ctx* c, int64_t cur);
int64_t kb_of(const pcoa_ctx* c, int64_t nv);
int64_t fp4_target_kb(const pcoa_ctx* c);
hipError_t launch_csr_operand(const pcoa_ctx* c, const int32_t* idx, const int64_t* offs, int64_t nv, int64_t offs_base,
                              int8_t* dst, hipStream_t s, int64_t kb);
int fp4_setup(pcoa_ctx* c);
int fp4_quiesce(pcoa_ctx* c);   // (operand.hip needs it ahead of its definition too: fold_if_needed -> fp4_quiesce -> fp4_resolve -> int8_chunk -> fold_if_needed)
int fp4_flush(pcoa_ctx* c);
int fp4_sync_point(pcoa_ctx* c);
int fp4_discard(pcoa_ctx* c);
int fp4_grow(pcoa_ctx* c, int bi, int64_t kb, int64_t chunk_variants);
int fp4_reserve(pcoa_ctx* c, int64_t kb, int64_t chunk_variants, int side_kind, bool verify, int8_t** dst,
                hipStream_t* stream, int32_t** flag);
void fp4_commit(pcoa_ctx* c, int64_t kb, int64_t vars);
int gram_device(pcoa_ctx* c, const void* x_dev, int is_u8, int64_t nv, int64_t ld, bool can_defer);
int gram_device_bits(pcoa_ctx* c, const uint32_t* bits_dev, int64_t nv, int64_t ld_words, bool can_defer);
int check_device_flags(pcoa_ctx* c);
int finalize_impl(pcoa_ctx* c);

// ---- reduce_peers.hip
// The partition of pcoa_gram_reduce_peers, stated once: with Q = ceil(N^2 / 4) quads of 16 bytes, owner g of k takes the quads
// [g Q / k, (g + 1) Q / k) (64-bit arithmetic) of the flat element range [0, N^2); *first / *count are in ELEMENTS, *first is a
// multiple of 4, and the last owner's count ends with the N^2 % 4 tail elements.  A chunk is empty when Q < k leaves it none.
void reduce_chunk(int32_t g, int32_t k, int32_t n, int64_t* first, int64_t* count);
// the matrices one chunk kernel sums, by value in the kernel's arguments: s32 of every engine, s64 where the engine has one
struct ReduceSources {
  const int32_t* s32[PCOA_REDUCE_MAX_ENGINES];
  const int64_t* s64[PCOA_REDUCE_MAX_ENGINES];
  int32_t k;
};
// dst[e] = sum over the sources of their element e, e in [first, first + count); dst may be one of the sources (the owner's own
// matrix: a lane reads an element before it writes it).  has64: some s64 entry is set
hipError_t launch_reduce_chunk_i32(const ReduceSources& src, int32_t* dst, int64_t first, int64_t count, hipStream_t stream);
hipError_t launch_reduce_chunk_i64(const ReduceSources& src, bool has64, int64_t* dst, int64_t first, int64_t count,
                                   hipStream_t stream);

// ---- capi_accumulate.hip
int csr_validate(pcoa_ctx* c);

// ---- row_feed.hip: the staging ring (protocol: StagingRing above)
int staging_acquire(pcoa_ctx* c, StagingRing& r, size_t need, size_t grow_to, StagingRing::Slot** out, size_t need1 = 0,
                    size_t grow_to1 = 0);
int staging_copied(pcoa_ctx* c, StagingRing::Slot& sl);
int staging_released(pcoa_ctx* c, StagingRing::Slot& sl, hipStream_t reader);
// hidden: shared between two translation units of the library and called from nowhere else, so it stays out of the dynamic symbols
__attribute__((visibility("hidden"))) int staging_pin(pcoa_ctx* c, StagingRing::Slot& sl, int i, size_t need, size_t grow_to);
int staging_wait_all(pcoa_ctx* c, StagingRing& r);
void staging_destroy(StagingRing& r);

// ---- capi_compute.hip
int ensure_workspace(pcoa_ctx* c, int32_t k);
int ensure_b(pcoa_ctx* c);
int lanczos_over(pcoa_ctx* c, int32_t num_pc, const LanczosMatvec& mv, double* out_components, double* out_eigenvalues,
                 int32_t* steps_out);

// ---- capi_measure.hip: the centring of c's measure (c->similarity != PCOA_SIMILARITY_SHARED) from the current S -- diagonal,
// row sums of K (from the upper-triangular tiles when sym_form: c->sym_part sized by the caller), stats, c->colmean, and B
// into b where b is not NULL.  measure_b: B alone, from the centring already there
int measure_centre(pcoa_ctx* c, bool sym_form, double* b);
int measure_b(pcoa_ctx* c, double* b);
void measure_bind(const pcoa_ctx* c, EigWorkspace* ws);   // ws->measure / diag / q from c
// a Jaccard / cosine measure is set or a call companion is bound: the three functions above serve both (a bound ctx goes to
// capi_complete.hip through them), the centring and the mat-vecs are not the shared count's
inline bool measured(const pcoa_ctx* c) { return c->similarity != PCOA_SIMILARITY_SHARED || c->companion != nullptr; }

// ---- capi_complete.hip: the same three for a ctx with a call companion (c->companion != nullptr)
int complete_centre(pcoa_ctx* c, bool sym_form, double* b);
int complete_b(pcoa_ctx* c, double* b);
void complete_bind(const pcoa_ctx* c, EigWorkspace* ws);
void complete_destroy(pcoa_ctx* c);   // the buffers, the events and an owned companion

// ---- capi_king.hip
void king_destroy(pcoa_ctx* c);   // the plane rows and the events, behind their last readers

// ---- capi_operator.hip
// words between two rows of c's store: carrier bitsets, or the 2-bit genotypes of a GRM ctx
inline int64_t store_pitch_words(const pcoa_ctx* c) { return c->is_grm ? grm_pitch_words(c->n) : operator_pitch_words(c->n); }
int store_grow(pcoa_ctx* c, int64_t nv);   // room for nv more rows, or PCOA_ERR_OUT_OF_MEMORY and the store as it was
// appends nv rows: repitch(done, cur, dst) queues the kernel that writes rows [done, done + cur) of the call at dst
int store_append(pcoa_ctx* c, int64_t nv, const std::function<hipError_t(int64_t, int64_t, uint32_t*)>& repitch);
int operator_append(pcoa_ctx* c, const uint32_t* bits_dev, int64_t nv, int64_t ld_words);
int operator_reset(pcoa_ctx* c);
int operator_reserve(pcoa_ctx* c, int32_t num_pc);
int operator_compute(pcoa_ctx* c, int32_t num_pc, double* out_components, double* out_eigenvalues, int32_t* out_nonzero_rows);
void operator_destroy(pcoa_ctx* c);
int64_t operator_store_bytes(const pcoa_ctx* c);

// ---- capi_grm.hip
int grm_accumulate_bed(pcoa_ctx* c, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes, int ref_is_a1, int source);
int grm_compute(pcoa_ctx* c, int32_t num_pc, double* out_components, double* out_eigenvalues, int32_t* out_nonzero_rows);
void grm_destroy(pcoa_ctx* c);
// the panel's resident per-variant parameters under its current min_maf, recomputed if the store or min_maf changed (the
// pointers stay valid until the store grows); *used_out = M'
struct GrmParams {
  const unsigned long long* mprime;
  const double *mu, *d;
  const int32_t* used;
};
int grm_resident_params(pcoa_ctx* c, GrmParams* out, int64_t* used_out);
int grm_resident_counts(pcoa_ctx* c);          // n_v, h_v, o_v of every row in c->grm_cnt, computed if the store changed
int grm_resident_weights(pcoa_ctx* c);         // and mu / d / used / M' under min_maf, the filters and an installed mask
const int32_t* grm_used_rows(const pcoa_ctx* c);   // used [V] of the resident weights
int64_t grm_store_ranges(const pcoa_ctx* c);   // ranges of kGrmRangeRows rows over the segments of c's store
// the counts, then mu / d / used / M' under the current min_maf WITHOUT the keep mask: *used_out[v] = 1 for a candidate of the LD
// prune.  The resident weights are marked stale where a mask is installed, so the next consumer computes them with it
int grm_unmasked_used(pcoa_ctx* c, const int32_t** used_out);
inline void grm_ld_drop(pcoa_ctx* c) {   // the keep mask no longer describes the store: the weights are the unpruned ones again
  if (c->grm_keep_set) c->grm_weights_set = false;
  c->grm_keep_set = false;
}

inline void grm_pcr_drop(pcoa_ctx* c, int32_t by) {   // the PC-Relate fit no longer describes the store
  if (c->grm_pcr_set) c->grm_pcr_dropped_by = by;
  c->grm_pcr_set = false;
}

// ---- capi_grm_project.hip
// the front of panel->grm_mw, in doubles: u [P][N] | lam [P] | t [P][V] | s [P][V] | tpart [2][groups][V] | the call's own part
struct GrmMultiWs {
  double *u, *lam, *t, *s, *tpart, *rest;
};
int grm_multi_ws(pcoa_ctx* panel, int32_t num_pc, int64_t rest_doubles, GrmMultiWs* w);
// t_c = D A u_c and s_c = -(mu t_c) of every component, two at a time, on the panel's stream (queued); eigenvalues (may be NULL:
// lam is then left as it is) travel with the components
int grm_panel_t(pcoa_ctx* panel, const GrmParams& g, const GrmMultiWs& w, int32_t num_pc, const double* components,
                const double* eigenvalues);

// ---- capi_grm_qc.hip
int grm_resident_hwe(pcoa_ctx* c);   // the counts, then p_v of every row in c->grm_hwe (resident until the counts change)
void grm_qc_destroy(pcoa_ctx* c);

// ---- capi_loadings.hip
void loadings_destroy(pcoa_ctx* c);

// ---- capi_ld.hip
void ld_destroy(pcoa_ctx* c);   // every buffer of the pruner (the ctx stream is idle)
void ld_drop_tail(pcoa_ctx* c); // the carried rows are forgotten (pcoa_ld_break, pcoa_reset)

struct ScopedTimer {
  pcoa_ctx* c;
  EventPair p;
  hipStream_t s;
  bool on;
  ScopedTimer(pcoa_ctx* ctx, int cat, hipStream_t stream = nullptr) : c(ctx), s(stream ? stream : ctx->stream), on(false) {
    p.a = get_event(c);
    p.b = get_event(c);
    p.cat = cat;
    if (p.a && p.b && hipEventRecord(p.a, s) == hipSuccess) on = true;
  }
  ~ScopedTimer() {
    if (on && hipEventRecord(p.b, s) == hipSuccess) {
      c->pending.push_back(p);
      if (c->pending.size() > 2048) drain_events(c, true);
    } else {
      if (p.a) c->pool.push_back(p.a);
      if (p.b) c->pool.push_back(p.b);
    }
  }
};

// *buf holds at least `need` elements (floor 1,024); its old contents are not kept
template <typename T>
int ensure(pcoa_ctx* c, T** buf, int64_t* cap, int64_t need) {
  if (need <= *cap) return PCOA_OK;
  *cap = 0;
  const int64_t newcap = std::max<int64_t>(need, 1024);
  const int rc = regrow(c, (void**)buf, sizeof(T) * (size_t)newcap, true);
  if (rc == PCOA_OK) *cap = newcap;
  return rc;
}

}  // namespace pcoa
