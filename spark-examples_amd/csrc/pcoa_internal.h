// Internal declarations shared by the HIP translation units of libpcoa_hip.so.
// gfx950 (MI355X / CDNA4) only: 64-wide wavefronts, MFMA, 160 KiB LDS per CU, 8 XCDs x 32 CUs.
#ifndef PCOA_INTERNAL_H_
#define PCOA_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "pcoa.h"

namespace pcoa {

constexpr int kWave = 64;     // CDNA wavefront
constexpr int kNumXcd = 8;    // MI355X: block b is dispatched to XCD b % 8 (speed only, never correctness)

// ---- debug / experiment knobs -------------------------------------------------------------------
// Every environment variable the library looks at, read ONCE (first use) into this struct; nothing else calls getenv.
// None is needed for normal use: they exist for tests and measurements; include/pcoa.h lists them.
struct DebugKnobs {
  int gram_kernel = -1;            // PCOA_GRAM_KERNEL = auto | fp4 | i8 | f32  -> 0 | 3 | 2 | 1 (overrides the create flags)
  int64_t pack_chunk = 0;          // PCOA_DEBUG_PACK_CHUNK: variants per pre-pass launch (tests: multi-chunk paths)
  int64_t max_launch = 0;          // PCOA_DEBUG_MAX_LAUNCH: variants per contraction launch (tests: multi-launch paths)
  int64_t fold_threshold = 0;      // PCOA_DEBUG_FOLD_THRESHOLD: int32 -> int64 fold (tests: the fold / int64 all-reduce)
  int pipeline = -1;               // PCOA_PIPELINE = 0 | 1: force the two-stream fp32 pipeline off / on where it fits
  int explicit_center = 0;         // PCOA_EXPLICIT_CENTER: materialise B for the Lanczos path
  int lockstep = -1;               // PCOA_GRAM_LOCKSTEP = 0 | 1: lock-step contraction launch off / on where it fits
  int guard = 0;                   // PCOA_DEBUG_GUARD = 1 | 2: every device buffer ends (1) / starts (2) at an unmapped page
  int kbits_mode = -1;             // PCOA_KBITS_MODE = 0 | 2 | 4 | 5: launch form of the k-bits contraction (whole chip)
  int symv_sym_min_n = 0;          // PCOA_SYMV_SYM_MIN_N: smallest N whose Lanczos mat-vec reads only the upper triangle of S (default 16384)
  int csr_legacy = 0;              // PCOA_CSR_LEGACY = 1: pcoa_accumulate_calls through the host-validated r03 path
  int kbits_w4 = -1;               // PCOA_KBITS_W4 = 0 | 1: one-wave-per-SIMD contraction (gram_kbits_w4.hip): 0 never, 1 wherever the kernel has its CUs to itself (default)
  int kbits_w4_diag = -1;          // PCOA_KBITS_W4_DIAG: 0 = diagonal tiles as in r04a (one wave idles), 1..16 = wave roles on diagonal tiles with this cost (of 16) in the even split; default 11
  int kbits_coreside = -1;         // PCOA_KBITS_CORESIDE = 0 | 1: fp32 pipeline with pre-pass and contraction on the SAME CUs (ring pre-pass)
  int bits_pipeline = 0;           // PCOA_BITS_PIPELINE = 1: bitset tiles through the co-resident pipeline as in r03 / r04 (default: transpose and contraction in series, the contraction as the one-wave-per-SIMD kernel)
  int lanczos_band_mmax = 0;       // PCOA_LANCZOS_BAND_MMAX: basis size of the band iteration (tests: forces thick restarts)
  int lanczos_band = 1;            // PCOA_LANCZOS_BAND = 0: no band-Lanczos fallback (r05 behaviour); 2: ONLY the band iteration (tests)
  int synth_tile = 0;              // PCOA_SYNTH_TILE = 1: pcoa_accumulate_synthetic through the fp32 staging tile + pre-pass (r05 path) instead of generating the k-bits operand directly
  int64_t operator_segment_rows = 0;  // PCOA_OPERATOR_SEGMENT_ROWS: rows per segment of an operator ctx's bit store (tests: segment boundaries with a few hundred rows)
  int64_t grm_segment_rows = 0;    // PCOA_GRM_SEGMENT_ROWS: the same for a GRM ctx's genotype store
  int no_narrow = 0;               // PCOA_NO_NARROW = 1: an int64 S that fits int32 stays int64 and pcoa_gram_reduce_from always widens (r05 behaviour; tests of the int64 kernels)
};
const DebugKnobs& debug_knobs();

// ---- Gram kernels, fp32 operand (gram_f32.hip) -------------------------------------------------
struct GramLaunch {
  const float* x;        // device, [nv][ld] carrier multiplicities (0/1)
  int64_t ld;
  int64_t nv;            // variants in this launch (<= 2^24 so fp32 accumulators stay exact)
  int32_t n;             // samples
  int32_t* s32;          // device, [n][n] int32 partial (upper-triangular tiles only)
  int32_t* flag;         // device: bit 4 is raised when an fp32 accumulator leaves the exact range (|sum| >= 2^24)
  const float* zeros;    // device, >= 4 KiB of zeros (source for out-of-range rows)
  int num_cu;
  hipStream_t stream;
};
// Returns hipSuccess or the launch error.  *splitk_out (optional) receives the split-K factor used.
hipError_t launch_gram_f32(const GramLaunch& g, int* splitk_out);

// ---- packed operands: a re-layout pre-pass into a k-blocked workspace, then the matrix-core contraction --------------
// Strip owner (SURVEY 8e, N beyond one HBM): the launch computes S[:, col0 .. col0 + cols) -- every row block against the
// column blocks of the strip, BOTH triangles -- into a row-major [n][cols] matrix.  cols == 0: the ordinary symmetric job.
struct GramStrip {
  int col0 = 0, cols = 0;
  int cb0 = 0;  // first column block (filled in by the launcher)
};

// shapes (gram_shape.hip).  gram_kb_pad: fmt 0 = int8 (16 variants per 16-byte lane slice), 1 = FP4 (32), 2 = k-bits
int64_t gram_packed_npad(int32_t n);
int64_t gram_packed_kb_pad_i8(int64_t nv);
size_t gram_packed_workspace_bytes(int32_t n, int64_t nv);
int64_t gram_kb_pad(int64_t nv, int fmt);
// Lock-step launch: all tiles of `splitk` k-streams resident at once, one workgroup per CU for the whole launch.
// gram_lockstep_splitk: the k-stream count that fits `cus` CUs (8 XCDs), 0 if the shape does not fit.
int gram_lockstep_splitk(int32_t n, int cus);
int gram_lockstep_workgroups(int32_t n, int splitk);

// pre-passes -> FP4 / int8 operand (pack_packed.hip)
// flag[0]: bit 2 = a value that is not an integer in [0, 127]; flag[1] = max value seen (atomicMax): the carrier
// multiplicity bound the host sizes its int32 launches and folds by
hipError_t launch_pack_f32_i8(const float* x, int64_t ld, int64_t nv, int32_t n, int8_t* p, int32_t* flag,
                              hipStream_t stream);
hipError_t launch_pack_u8_i8(const uint8_t* x, int64_t ld, int64_t nv, int32_t n, int8_t* p, int32_t* flag,
                             hipStream_t stream);
hipError_t launch_densify_csr_i8(const int32_t* idx_dev, const int64_t* offs_dev, int64_t nv, int64_t offs_base,
                                 int8_t* p, int32_t n, int32_t* flag, hipStream_t stream);
// FP4 (MX E2M1) variant: fmt 1 = 32 variants per 16-byte lane slice, values must be exactly 0 / 1
hipError_t launch_densify_csr_fp4(const int32_t* idx_dev, const int64_t* offs_dev, int64_t nv, int64_t offs_base,
                                  int8_t* p, int32_t n, int32_t* flag, hipStream_t stream, int64_t nkb_out);
hipError_t launch_expand_bits_fp4(const uint32_t* bits, int64_t ld_words, int64_t nv, int32_t n, int8_t* p,
                                  hipStream_t stream, int64_t nkb_out = 0);
hipError_t launch_pack_fp4(const void* x, int is_u8, int64_t ld, int64_t nv, int32_t n, int8_t* p, int32_t* flag,
                           hipStream_t stream, int64_t nkb_out = 0);
// fp32 tiles the LDS-DMA-ring pre-passes take: ld % 4 == 0 and a 16-byte aligned base
bool pack_fp4_ring_ok(const void* x, int64_t ld);

// contraction of an FP4 (fmt 1) / int8 (fmt 0) operand (gram_packed.hip)
// skip (optional, device): the launch does nothing when *skip != 0 -- the auto mode's device-side predicate (a pre-pass
// found a value other than 0 / 1 in the buffered tiles; the host learns it later and redoes them on the int8 kernel)
hipError_t launch_gram_packed(const int8_t* p, int fmt, int64_t nv, int32_t n, int32_t* s32, int num_cu,
                              hipStream_t stream, int* splitk_out, const int32_t* skip = nullptr,
                              GramStrip strip = GramStrip{});
hipError_t launch_gram_packed_lockstep(const int8_t* p, int fmt, int64_t nv, int32_t n, int32_t* s32, int num_cu,
                                       hipStream_t stream, const int32_t* skip = nullptr);

// pre-passes -> k-bits operand (pack_kbits.hip): K1[V/128][Npad][4 words], one BIT per genotype, expanded to FP4 in
// registers by the contraction.  nblk_out = blocks of 128 variants to write (the tail beyond nv is zero-filled).
hipError_t launch_pack_kbits(const void* x, int is_u8, int64_t ld, int64_t nv, int32_t n, int8_t* p, int32_t* flag,
                             hipStream_t stream, int64_t nblk_out);
hipError_t launch_transpose_bits_kbits(const uint32_t* bits, int64_t ld_words, int64_t nv, int32_t n, int8_t* p,
                                       hipStream_t stream, int64_t nblk_out);
hipError_t launch_densify_csr_kbits(const int32_t* idx_dev, const int64_t* offs_dev, int64_t nv, int64_t offs_base,
                                    int8_t* p, int32_t n, int32_t* flag, hipStream_t stream, int64_t nblk_out);
// persistent LDS-DMA-ring form of the fp32 -> k-bits pre-pass (needs pack_fp4_ring_ok): <= wgs workgroups, 8 rows in flight
// per wave, default cache policy
hipError_t launch_pack_kbits_ring(const float* x, int64_t ld, int64_t nv, int32_t n, int8_t* p, int32_t* flag,
                                  hipStream_t stream, int64_t nblk_out, int wgs);
// the uint8 form: units of 128 variants x 1,024 samples, one wave per SIMD (ld % 8 == 0, 8-byte aligned base)
bool pack_u8_ring_ok(const void* x, int64_t ld);
hipError_t launch_pack_kbits_ring_u8(const uint8_t* x, int64_t ld, int64_t nv, int32_t n, int8_t* p, int32_t* flag,
                                     hipStream_t stream, int64_t nblk_out, int wgs);

// contraction of a k-bits operand, two waves per SIMD (gram_kbits.hip); mode 0 = split-K launch, 2 = lock-step, 4 = even split
// of the (tile, stage) units over num_cu workgroups
hipError_t launch_gram_kbits(const int8_t* p, int64_t nv, int32_t n, int32_t* s32, int num_cu, hipStream_t stream, int mode,
                             const int32_t* skip = nullptr, GramStrip strip = GramStrip{});
// the same contraction with one wave per SIMD and 128 x 128 wave tiles (gram_kbits_w4.hip); same modes
hipError_t launch_gram_kbits_w4(const int8_t* p, int64_t nv, int32_t n, int32_t* s32, int num_cu, hipStream_t stream, int mode,
                                const int32_t* skip = nullptr, GramStrip strip = GramStrip{}, int wdiag = -1);

// ---- auxiliary Gram kernels (gram_aux.hip) ----------------------------------------------------
hipError_t launch_densify_csr(const int32_t* idx_dev, const int64_t* offs_dev, int64_t v0, int64_t nv,
                              int64_t offs_base, float* x_dev, int64_t ld, int32_t n, int32_t* err_flag_dev,
                              hipStream_t stream);
// a one-wave spin (fp32 pipeline: head start for the contraction, operand.hip fp4_setup)
hipError_t launch_delay_us(hipStream_t stream, int microseconds);
hipError_t launch_symmetrize_i32(int32_t* s32, int32_t n, hipStream_t stream);
hipError_t launch_fold_i32_to_i64(int32_t* s32, int64_t* s64, int64_t count, hipStream_t stream);
hipError_t launch_export_i64(const int32_t* s32, const int64_t* s64_or_null, int64_t* dst, int64_t count,
                             hipStream_t stream);
hipError_t launch_plink_bed_to_bits(const uint8_t* bed, int64_t row_bytes, int64_t nv, int32_t n, int64_t words, int ref_a1,
                                    uint32_t* bits, hipStream_t stream);
hipError_t launch_add_i64(int64_t* dst, const int64_t* src, int64_t count, hipStream_t stream);
hipError_t launch_add_i32(int32_t* dst, const int32_t* src, int64_t count, hipStream_t stream);
// s32[i] = (int32) s64[i] where it fits; flag[0] != 0 if some entry does not; ((int64*)flag)[1] = max |entry| (flag: 16 zeroed bytes)
hipError_t launch_narrow_i64_to_i32(const int64_t* s64, int32_t* s32, int64_t count, int32_t* flag, hipStream_t stream);
hipError_t launch_synth_fill_f32(uint64_t seed, const uint32_t* thresholds_dev, const int32_t* sample_pop_dev,
                                 int32_t n_pops, int64_t first_variant, int64_t nv, int32_t n, float* x_dev,
                                 int64_t ld, hipStream_t stream);

// the same genotypes straight into the k-bits operand (nblk_out blocks of 128 variants, the tail beyond nv zero; n_pops <= 64,
// nblk_out <= 65,535); thresholds_dev: [nv][n_pops] of exactly this range
hipError_t launch_synth_kbits(uint64_t seed, const uint32_t* thresholds_dev, const int32_t* sample_pop_dev, int32_t n_pops,
                              int64_t first_variant, int64_t nv, int32_t n, int32_t npad, int8_t* p, int64_t nblk_out,
                              hipStream_t stream);

// ---- S of a sample subset (subset.hip): dst[a][b] = src[keep[a]][keep[b]], dst [m][m], src [n][n], keep_dev m strictly
// increasing indices in [0, n) on the device (the caller validates them).  A workgroup takes kSubsetBandRows dst rows x
// kSubsetTileCols dst columns; every entry of dst is written exactly once
constexpr int32_t kSubsetTileCols = 1024;
constexpr int32_t kSubsetBandRows = 32;
hipError_t launch_subset_gather_i32(const int32_t* src, int32_t n, const int32_t* keep_dev, int32_t m, int32_t* dst,
                                    hipStream_t stream);
hipError_t launch_subset_gather_i64(const int64_t* src, int32_t n, const int32_t* keep_dev, int32_t m, int64_t* dst,
                                    hipStream_t stream);

// ---- the screen for duplicate and related pairs (pairs.hip): pair (i, j), i < j, is reported iff U = d_i + d_j - S(i, j) > 0 and
// (double)S(i, j) >= x * (double)U, d = the diagonal of S.  A workgroup takes kPairsBandRows rows x kPairsTileCols columns.
// All buffers are the caller's, on the device of s32: diag n int64; cnt n * pairs_tiles(n) int32 (the counts, then their
// exclusive prefix within each row); rowoff n + 1 int64 (row totals, then their exclusive prefix; rowoff[n] = n_found)
constexpr int32_t kPairsTileCols = 1024;
constexpr int32_t kPairsBandRows = 32;
constexpr int32_t kPairsMaxSamples = 1 << 30;   // column arithmetic stays inside int32 with a tile to spare
int32_t pairs_tiles(int32_t n);
int64_t pairs_count_pass_entries(int32_t n);   // entries of S the count pass loads (pure function of n)
hipError_t launch_pairs_diag(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int64_t* diag, hipStream_t stream);
hipError_t launch_pairs_count(const int32_t* s32, const int64_t* s64_or_null, int32_t n, const int64_t* diag, double x,
                              int32_t* cnt, hipStream_t stream);
hipError_t launch_pairs_scan(int32_t* cnt, int32_t n, int64_t* rowoff, hipStream_t stream);   // both scans
// the row scan alone, over any [rows][ntiles] counts: cnt[r][.] := its exclusive prefix, rowoff[r] := the row's total
hipError_t launch_pairs_row_scan(int32_t* cnt, int32_t rows, int32_t ntiles, int64_t* rowoff, hipStream_t stream);
// out[p] for the list positions p < capacity (capacity >= 1 entries allocated), in increasing (i, j) order.  *entries_read
// (optional, zeroed by the caller) grows by the entries of S the pass reads again: the widths of the (row, tile) cells it visits
hipError_t launch_pairs_write(const int32_t* s32, const int64_t* s64_or_null, int32_t n, const int64_t* diag, double x,
                              const int32_t* prefix, const int64_t* rowoff, int64_t capacity, pcoa_pair* out,
                              unsigned long long* entries_read, hipStream_t stream);

// ---- the KING-robust kinship screen over five Gram matrices (king.hip; the rule is stated at the top of that file).  The
// matrices and the decode's five output buffers travel by value in the kernels' arguments, indexed by PCOA_KING_*.  The grid,
// cnt and rowoff are the pairs screen's (pairs_tiles, launch_pairs_scan).  flag: four int32 words zeroed by the caller, one per
// consistency check; h, hm: n int64 each; v: one int64 (V), written by the diagonal kernel and read by the two passes
struct KingMatrices { const int32_t* p[PCOA_KING_PLANES]; };
struct KingPlaneRows { uint32_t* p[PCOA_KING_PLANES]; };
constexpr int kKingFlagV = 0, kKingFlagIbs0 = 1, kKingFlagHetSum = 2, kKingFlagSHm = 3, kKingFlagWords = 4;
// PLINK .bed rows -> the five class bitsets (dense rows of `words` words, samples >= n masked in every plane), one read
hipError_t launch_plink_bed_to_king_planes(const uint8_t* bed, int64_t row_bytes, int64_t nv, int32_t n, int64_t words,
                                           const KingPlaneRows& out, hipStream_t stream);
hipError_t launch_king_diag(const KingMatrices& g, int32_t n, int64_t* h, int64_t* hm, int64_t* v, int32_t* flag, hipStream_t stream);
hipError_t launch_king_count(const KingMatrices& g, int32_t n, const int64_t* h, const int64_t* hm, const int64_t* v, double x,
                             int32_t* cnt, int32_t* flag, hipStream_t stream);
hipError_t launch_king_write(const KingMatrices& g, int32_t n, const int64_t* h, const int64_t* hm, const int64_t* v, double x,
                             const int32_t* prefix, const int64_t* rowoff, int64_t capacity, pcoa_king_pair* out,
                             unsigned long long* entries_read, hipStream_t stream);

// ---- implicit similarity operator (operator_bits.hip): y = X^T (X v) from the carrier bitsets, S never formed -------------
// The store is a list of segments, each rows x operator_pitch_words(n) words; bits of samples >= n and the pitch's padding are
// zero.  A product's additions are ordered by sample group (kOperatorGroupWords word columns), segment and range of
// kOperatorRangeRows rows -- never by the grid.
constexpr int32_t kOperatorRangeRows = 512;    // rows of a segment whose pass-2 partial vector one wave accumulates in order
constexpr int32_t kOperatorSegmentAlign = 2048;   // a segment that holds this many rows holds a whole multiple of them (whole ranges)
constexpr int32_t kOperatorGroupWords = 256;   // word columns (8,192 samples) a pass-1 workgroup reduces before it writes
int32_t operator_pitch_words(int32_t n);
int32_t operator_groups(int32_t n);
hipError_t launch_operator_append(const uint32_t* src, int64_t ld_words, int64_t nv, int32_t n, uint32_t* dst, hipStream_t stream);
// tpart[g * vstride + r] = the part of (X v)[r] from sample group g, r in [0, rows) of this segment
hipError_t launch_operator_xv(const uint32_t* seg, int32_t rows, int32_t n, const double* v, double* tpart, int64_t vstride,
                              hipStream_t stream);
hipError_t launch_operator_combine_t(const double* tpart, int64_t vstride, int32_t n, int64_t rows, double* t, hipStream_t stream);
// ypart[q * pitch * 32 + i] = sum over the rows r of range q of this segment of bit(r, i) t[r]; ceil(rows / range) ranges
hipError_t launch_operator_xt_f64(const uint32_t* seg, int32_t rows, int32_t n, const double* t, double* ypart, hipStream_t stream);
hipError_t launch_operator_xt_i64(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* cnt, int64_t* ipart,
                                  hipStream_t stream);
hipError_t launch_operator_popcount(const uint32_t* seg, int32_t rows, int32_t n, int32_t* cnt, hipStream_t stream);
// dots[0] = 1^T v, dots[1] = means^T v
hipError_t launch_operator_dots(const double* v, const double* means, int32_t n, double* dots, hipStream_t stream);
// y = the ranges' partials added in order; centred: ((y - means (1^T v)) - means^T v) + stats[1] (1^T v)
hipError_t launch_operator_finish(const double* ypart, int32_t nranges, int32_t n, const double* means, const double* stats,
                                  const double* dots, int centred, double* y, hipStream_t stream);
hipError_t launch_operator_row_sums_finish(const int64_t* ipart, int32_t nranges, int32_t n, int64_t* rs_i64, double* rs_f64,
                                           hipStream_t stream);

// ---- standardised-genotype operator (grm_bits.hip): y = A^T diag(d) A x / M' from 2-bit genotype rows, K never formed ------
// The store is a list of segments, each rows x grm_pitch_words(n) words of 16 genotypes in one coding (00 g = 0, 01 not called,
// 10 g = 1, 11 g = 2); slots of samples >= n and the pitch's padding hold 01.  A product's additions are ordered by sample group
// (kGrmGroupWords word columns), segment and range of kGrmRangeRows rows -- never by the grid.
constexpr int32_t kGrmRangeRows = 512;       // rows of a segment whose pass-2 partial vector one wave accumulates in order
constexpr int32_t kGrmSegmentAlign = 2048;   // a segment that holds this many rows holds a whole multiple of them (whole ranges)
constexpr int32_t kGrmGroupWords = 256;      // word columns (4,096 samples) a pass-1 workgroup reduces before it writes
int32_t grm_pitch_words(int32_t n);
int32_t grm_groups(int32_t n);
// raw .bed rows -> store rows; swap: exchange 00 and 11 (the non-reference allele is A1)
hipError_t launch_grm_append(const uint8_t* src, int64_t row_bytes, int64_t nv, int32_t n, int swap, uint32_t* dst, hipStream_t stream);
// cnt[r * 3 + {0, 1, 2}] = called, het, hom non-reference of row r
hipError_t launch_grm_counts(const uint32_t* seg, int32_t rows, int32_t n, int32_t* cnt, hipStream_t stream);
// mu, d, used per variant; *mprime (zeroed by the caller) += the used variants.  keep: NULL, or [rows] bytes of an LD keep mask
// (0: the row is not used whatever its counts say).  n, max_missing, hwe_min_p, hwe_p (NULL, or [rows] p-values of launch_grm_hwe):
// the variant filters of pcoa_grm_set_variant_filters
hipError_t launch_grm_weights(const int32_t* cnt, int64_t rows, double min_maf, const uint8_t* keep, int32_t n, double max_missing,
                              double hwe_min_p, const double* hwe_p, double* mu, double* d, int32_t* used,
                              unsigned long long* mprime, hipStream_t stream);
// tpart[g * vstride + r] = the part of (A x)[r] from sample group g, r in [0, rows) of this segment (mu: the segment's first row)
hipError_t launch_grm_ax(const uint32_t* seg, int32_t rows, int32_t n, const double* mu, const double* x, double* tpart,
                         int64_t vstride, hipStream_t stream);
// t = d * (the groups' partials in order), s = -(mu t)
hipError_t launch_grm_combine_t(const double* tpart, int64_t vstride, int32_t n, int64_t rows, const double* mu, const double* d,
                                double* t, double* s, hipStream_t stream);
// ypart[q * pitch * 16 + i] = sum over the rows r of range q of this segment of g(r, i) t[r] + c(r, i) s[r]
hipError_t launch_grm_at(const uint32_t* seg, int32_t rows, int32_t n, const double* t, const double* s, double* ypart,
                         hipStream_t stream);
// the same over c(r, i) used[r], int32
hipError_t launch_grm_called(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* used, int32_t* ipart, hipStream_t stream);
// y = the ranges' partials added in order, over M' (M' = 0: y = 0)
hipError_t launch_grm_finish(const double* ypart, int32_t nranges, int32_t n, const unsigned long long* mprime, double* y,
                             hipStream_t stream);
// *nz (zeroed by the caller) += the samples whose summed partials are positive
hipError_t launch_grm_called_finish(const int32_t* ipart, int32_t nranges, int32_t n, int32_t* nz, hipStream_t stream);

// ---- quality control on the store (grm_qc.hip) -----------------------------------------------------------------
// p[r] = the Hardy-Weinberg exact-test p-value of row r from cnt[r * 3 + {0, 1, 2}] (the rule: pcoa.h at pcoa_grm_hwe)
hipError_t launch_grm_hwe(const int32_t* cnt, int64_t rows, double* p, hipStream_t stream);
// fails[0 .. 3) (zeroed by the caller) += the rows that fail the MAF, the missing and the HWE test, each judged alone
hipError_t launch_grm_qc_fails(const int32_t* cnt, int64_t rows, int32_t n, double min_maf, double max_missing, double hwe_min_p,
                               const double* hwe_p, unsigned long long* fails, hipStream_t stream);
// ipart[(q * 3 + class) * pitch * 16 + i] = the rows r of range q of this segment, used[r] != 0 where used is given, at which
// sample i is missing (class 0), heterozygous (1), homozygous non-reference (2)
hipError_t launch_grm_sample_counts(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* used, int32_t* ipart,
                                    hipStream_t stream);
// out[i * 3 + {0, 1, 2}] = rows_counted - missing, het, hom: the ranges' partials added in order, int64
hipError_t launch_grm_sample_counts_finish(const int32_t* ipart, int32_t nranges, int32_t n, int64_t rows_counted, int64_t* out,
                                           hipStream_t stream);

// ---- the two passes for k vectors at once (grm_multi.hip): SNP weights and the projection of new samples ------
// k must be 1 or 2 (grm_multi_chunk picks the chunk).  Every column is added in the order of the one-vector kernels, so column c
// of any chunk has the bits of a one-vector run.
int grm_multi_chunk(int32_t remaining);
// tpart[c * cstride + g * vstride + r] = the part of (A x_c)[r] from sample group g; x_c = x + c * xstride, c in [0, k)
hipError_t launch_grm_ax_multi(const uint32_t* seg, int32_t rows, int32_t n, const double* mu, const double* x, int64_t xstride, int32_t k,
                               double* tpart, int64_t vstride, int64_t cstride, hipStream_t stream);
// ypart[c * cstride + q * pitch * 16 + i] = sum over the rows r of range q of g(r, i) t_c[r] + c(r, i) s_c[r]; t_c = t + c * tstride,
// s_c = s + c * tstride
hipError_t launch_grm_at_multi(const uint32_t* seg, int32_t rows, int32_t n, const double* t, const double* s, int64_t tstride, int32_t k,
                               double* ypart, int64_t cstride, hipStream_t stream);
// out[c * n + i] = (the ranges' partials of column c added in order) / M' / lam[c], c in [0, k)
hipError_t launch_grm_project_finish(const double* ypart, int32_t nranges, int64_t cstride, int32_t n, int32_t k,
                                     const unsigned long long* mprime, const double* lam, double* out, hipStream_t stream);
// called[i] = the ranges' integer partials added
hipError_t launch_grm_called_sum(const int32_t* ipart, int32_t nranges, int32_t n, int32_t* called, hipStream_t stream);
// out[v * num_pc + c] for the rows [first, first + nv): t_c[first + v], or with scaled the unit weight
// used ? t / sqrt(d * ((double)M' * lam[c])) : 0.0
hipError_t launch_grm_weights_out(const double* t, int64_t tstride, const double* d, const int32_t* used,
                                  const unsigned long long* mprime, const double* lam, int scaled, int64_t first, int64_t nv,
                                  int32_t num_pc, double* out, hipStream_t stream);

// ---- the least-squares projection (grm_lsq.hip): the normal equations H_q x = P_q of every study sample ------
constexpr int32_t kGrmLsqMaxPc = 16;      // 136 pair sums
constexpr int32_t kGrmLsqMaxChunk = 4;    // pairs one pass over the study's store carries
int grm_lsq_chunk(int32_t remaining);     // 4, 2 or 1
// p[j * rows + v] = used[v] ? (t_c[v] * t_c'[v]) / d[v] : 0.0 for the pairs e = e0 + j, j in [0, nj), e = c (c + 1) / 2 + c', c' <= c
hipError_t launch_grm_lsq_products(const double* t, int64_t tstride, const double* d, const int32_t* used, int64_t rows, int32_t e0,
                                   int32_t nj, double* p, hipStream_t stream);
// hpart[j * cstride + q * pitch * 16 + i] = sum over the rows r of range q of c(r, i) p_j[r]; p_j = p + j * pstride, nj in {1, 2, 4}
hipError_t launch_grm_lsq_pairs(const uint32_t* seg, int32_t rows, int32_t n, const double* p, int64_t pstride, int32_t nj, double* hpart,
                                int64_t cstride, hipStream_t stream);
// out[c * n + i] = the ranges' partials of column c added in order, c in [0, k): nothing is divided
hipError_t launch_grm_lsq_finish(const double* part, int32_t nranges, int64_t cstride, int32_t n, int32_t k, double* out,
                                 hipStream_t stream);
// a: [num_pc (num_pc + 1) / 2 + num_pc][nq], H packed then P; solved in place, the coordinates replace P (NaN, determined[q] = 0
// and *undetermined += 1 for a sample the rule of pcoa.h calls undetermined)
hipError_t launch_grm_lsq_solve(double* a, int32_t nq, int32_t num_pc, int32_t* determined, int32_t* undetermined, hipStream_t stream);

// ---- reading K out (grm_dense.hip): a rectangle of num(i, j) = sum_v (d_v a_v,lo) a_v,hi and of n(i, j) -------------
// One launch per segment, in the store's order.  out_k / out_n: [nrows][ncols] row-major, either may be NULL (that pass is not
// instantiated); first = 1: the entries start from 0, otherwise from what out_k / out_n hold.  mu, d, used: the segment's rows.
hipError_t launch_grm_dense(const uint32_t* seg, int32_t rows, int32_t n, const double* mu, const double* d, const int32_t* used,
                            int32_t row0, int32_t nrows, int32_t col0, int32_t ncols, int first, double* out_k, int32_t* out_n,
                            hipStream_t stream);
// k[i] = divisor 0: k[i] / M'; divisor 1: n[i] > 0 ? k[i] / n[i] : 0.0
hipError_t launch_grm_dense_finish(double* k, const int32_t* n, int64_t total, int32_t divisor, int64_t mprime, hipStream_t stream);

// ---- the relatedness cut-off on K (grm_pairs.hip): the screen of one row band of K as launch_grm_dense /
// launch_grm_dense_finish leave it.  k (and nb, the pair counts, or NULL): rows [r0, r0 + nrows) of K x columns [c0, c0 + pitch)
// at `pitch` elements a row, c0 a multiple of 64 at or below r0, pitch >= n - c0; a pitch that is a multiple of 4 on a 16-byte
// aligned k takes the 16-byte loads.  A workgroup takes kGrmPairsRows rows x kGrmPairsTileCols columns.  cnt: nrows *
// grm_pairs_tiles(n - c0) int32; rowoff: nrows + 1 int64; total_io: one int64, the pairs of the bands before on entry and with
// this band's on exit (the list position the band's first pair takes)
constexpr int32_t kGrmPairsTileCols = 1024;
constexpr int32_t kGrmPairsRows = 64;
int32_t grm_pairs_tiles(int32_t width);
int64_t grm_pairs_count_pass_entries(int32_t r0, int32_t nrows, int32_t c0, int32_t n);   // entries the count pass loads
// cnt[row][tile] = the columns j > i of the tile with K >= cutoff; diag_or_null[i] = K(i, i) for the band's rows
hipError_t launch_grm_pairs_count(const double* k, int64_t pitch, int32_t r0, int32_t nrows, int32_t c0, int32_t n, double cutoff,
                                  int32_t* cnt, double* diag_or_null, hipStream_t stream);
hipError_t launch_grm_pairs_scan(int32_t* cnt, int32_t nrows, int32_t ntiles, int64_t* rowoff, int64_t* total_io, hipStream_t stream);
// out[p] for the list positions p < capacity; n of a record = nb's entry, or mprime where nb is NULL.  *entries_read (optional,
// zeroed by the caller) grows by the entries of the band the pass reads again
hipError_t launch_grm_pairs_write(const double* k, const int32_t* nb_or_null, int64_t pitch, int32_t r0, int32_t nrows, int32_t c0,
                                  int32_t n, double cutoff, int64_t mprime, const int32_t* prefix, const int64_t* rowoff,
                                  int64_t capacity, pcoa_grm_pair* out, unsigned long long* entries_read, hipStream_t stream);

// ---- the KING-robust screen on the 2-bit store (grm_king.hip) ----------------------------------------------------
// A rectangle of hethet / ibs0 / het_sum (the rule: pcoa.h at pcoa_grm_king_block) as four int8 products on the matrix cores.  One
// launch per segment; outputs [nrows][ncols] row-major int32, any may be NULL, not all; first = 1: the entries are stored,
// otherwise added to what the outputs hold.  used_or_null: the segment's used_v, a row with 0 counts as all-missing
hipError_t launch_grm_king_counts(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* used_or_null, int32_t row0, int32_t nrows,
                                  int32_t col0, int32_t ncols, int first, int32_t* out_hethet, int32_t* out_ibs0, int32_t* out_het_sum,
                                  hipStream_t stream);
// the screen of one row band of the three counts, laid out as launch_grm_pairs_count's band (pitch a multiple of 4, the arrays
// 16-byte aligned); cnt / rowoff / total_io and the scans are launch_grm_pairs_scan's.  het_or_null[i] = hethet(i, i) = h_i
hipError_t launch_grm_king_screen_count(const int32_t* hethet, const int32_t* ibs0, const int32_t* het_sum, int64_t pitch, int32_t r0,
                                        int32_t nrows, int32_t c0, int32_t n, double x, int32_t* cnt, int64_t* het_or_null,
                                        hipStream_t stream);
hipError_t launch_grm_king_screen_write(const int32_t* hethet, const int32_t* ibs0, const int32_t* het_sum, int64_t pitch, int32_t r0,
                                        int32_t nrows, int32_t c0, int32_t n, double x, const int32_t* prefix, const int64_t* rowoff,
                                        int64_t capacity, pcoa_king_pair* out, unsigned long long* entries_read, hipStream_t stream);

// ---- PC-Relate kinship on the 2-bit store (grm_pcrelate.hip) ---------------------------------------------------------
// A rectangle of num / den / n (the rule: pcoa.h at pcoa_grm_pcrelate_block) as three fp64 products on the matrix cores.  One
// launch per segment, in the store's order; out_num, out_den: [nrows][ncols] row-major, out_n the same in int32 or NULL (that
// product is not instantiated); first = 1: the entries start from 0, otherwise from what the outputs hold.  used, beta
// ([rows][n_cov]): the segment's rows; basis: [n_cov][n]; t: the threshold on mu_iv.  The kernel is instantiated for
// grm_pcrelate_padded_cov(n_cov) covariates: 1, 3, 5 or 9
constexpr int32_t kGrmPcrelateMaxCov = 9;
int32_t grm_pcrelate_padded_cov(int32_t n_cov);
hipError_t launch_grm_pcrelate(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* used, const double* beta, int32_t n_cov,
                               const double* basis, double t, int32_t row0, int32_t nrows, int32_t col0, int32_t ncols, int first,
                               double* out_num, double* out_den, int32_t* out_n, hipStream_t stream);
// num[i] = den[i] > 0 ? num[i] / (4.0 * den[i]) : 0.0
hipError_t launch_grm_pcrelate_finish(double* num, const double* den, int64_t total, hipStream_t stream);
// beta[r * n_cov + c0 + c] = (the groups' partials tpart[c * cstride + g * vstride + r] of launch_grm_ax_multi added in group order)
// + mu[r] * s[c0 + c], c in [0, k), r in [0, rows)
hipError_t launch_grm_pcrelate_beta(const double* tpart, int64_t vstride, int32_t n, int64_t cstride, int64_t rows, const double* mu,
                                    const double* s, int32_t c0, int32_t k, int32_t n_cov, double* beta, hipStream_t stream);
// out[(v - first) * n + i] = mu_iv for the rows [first, first + nv) of beta, unmasked
hipError_t launch_grm_pcrelate_isaf(const double* beta, int32_t n_cov, const double* basis, int32_t n, int64_t first, int64_t nv,
                                    double* out, hipStream_t stream);

// ---- per-variant loadings (loadings.hip): out[v * num_pc + c] = (sum_i bit(v, i) u[c * ustride + i]) / div[c] for c in [0, k) ----
// u: prepared vectors, ustride = 32 ceil(n / 32) doubles each, zero for i >= n (that is what ignores a row's tail bits); div: k
// divisors or NULL; k must be 1, 2, 4 or 8 (loadings_chunk picks the chunk); out / u / div point at the chunk's first component.
// loadings_lanes(n): lanes that share a row (8, 16, 32 or 64) -- with n, all that the order of an entry's additions depends on
int32_t loadings_lanes(int32_t n);
int loadings_chunk(int32_t remaining);
hipError_t launch_loadings(const uint32_t* bits, int64_t nv, int64_t ld_words, int32_t n, const double* u, int64_t ustride, int32_t k,
                           const double* div, double* out, int32_t num_pc, hipStream_t stream);

// ---- LD pruning (ld.hip): the kernels of pcoa_ld_* over the pruner's work buffer -- [window + C][ceil(n / 32)] dense rows, the
// carried tail in front of the chunk's rows, and the carrier counts laid out the same way (wb_rows / cnt_rows: the chunk's
// first row, wb / cnt: the buffer's).  tail: carried rows that exist (<= window); ex: [vc][ceil(window / 32)] band words, bit
// d - 1 of a row set where the row at distance d exists and exceeds t; g0: rows fed since the last break; flags: 64 words; kbits:
// [vc / 32 + 2] keep flags as the resolve wave holds them ----
int32_t ld_band_tile_rows();     // target rows a band workgroup owns
int32_t ld_band_chunk_words();   // words of the sample axis it stages at a time
hipError_t launch_ld_count(const uint32_t* rows, int64_t ld, int64_t vc, int32_t n, uint32_t* wb_rows, int32_t* cnt_rows,
                           hipStream_t stream);
hipError_t launch_ld_band(const uint32_t* wb, const int32_t* cnt, int64_t vc, int32_t n, int32_t window, int32_t tail, double t,
                          uint32_t* ex, hipStream_t stream);
hipError_t launch_ld_resolve(const uint32_t* ex, const int32_t* cnt_rows, int64_t vc, int32_t n, int32_t window, int64_t g0,
                             uint32_t* flags, uint32_t* kbits, hipStream_t stream);
hipError_t launch_ld_scan(const uint32_t* kbits, int64_t g0, const int32_t* cnt_rows, int64_t vc, int32_t n, uint8_t* keep,
                          int32_t* pos, int64_t* out2, hipStream_t stream);
hipError_t launch_ld_gather(const uint32_t* wb_rows, const uint8_t* keep, const int32_t* pos, int64_t vc, int32_t n, uint32_t* out,
                            hipStream_t stream);

// ---- LD pruning of the GRM store by dosage r^2 (grm_ld.hip).  wb: [window + vc][grm_pitch_words(n)] store rows,
// the chunk's first row at row `window`, the rows in front of it before that; reach[r]: the distances at which an earlier row
// exists for chunk row r (<= window; breaks: sorted global row indices on the device, g0: the global index of the chunk's first
// row); ex: band words in launch_ld_band's format, so launch_ld_resolve / launch_ld_scan take them as they are ----
int32_t grm_ld_band_tile_rows();        // target rows a band workgroup owns
int32_t grm_ld_band_chunk_samples();    // samples of the sample axis it stages at a time
hipError_t launch_grm_ld_reach(const int64_t* breaks, int64_t n_breaks, int64_t g0, int64_t vc, int32_t window, int32_t* reach,
                               hipStream_t stream);
hipError_t launch_grm_ld_band(const uint32_t* wb, const int32_t* reach, int64_t vc, int32_t n, int32_t window, double t, uint32_t* ex,
                              hipStream_t stream);

// ---- sample subsets of the GRM store (grm_subset.hip): rows x grm_pitch_words(n_src) words -> rows x
// grm_pitch_words(n_keep) words, slot a of a row = slot keep[a] of the source row, 01 behind n_keep.  keep: n_keep device indices,
// strictly increasing, inside [0, n_src) (checked by the caller) ----
int32_t grm_subset_tile_rows();   // rows a lane keeps in flight
hipError_t launch_grm_subset(const uint32_t* src, int64_t rows, int32_t n_src, const int32_t* keep, int32_t n_keep, uint32_t* dst,
                             int32_t num_cu, hipStream_t stream);

// ---- centring (center.hip) --------------------------------------------------------------------
// s = s32 + (s64 ? s64 : 0).  row_sums[n] (fp64), stats[0] = matrix sum, stats[1] = matrix mean,
// nz[0] = #rows with sum > 0.  b = centred matrix fp64 [n][n].
// cm[j] = rowSums(j) / N (the division center_kernel performs per entry, done once)
hipError_t launch_col_means(const double* row_sums, int32_t n, double* cm, hipStream_t stream);
hipError_t launch_center(const int32_t* s32, const int64_t* s64_or_null, int32_t n, double* row_sums,
                         double* stats, int32_t* nz, double* b, hipStream_t stream, bool row_sums_done = false);

// ---- strip owner reductions (center.hip): S is [n][cols], column jj = sample col0 + jj
// ws: strip_ws_doubles(n, cols) doubles; the result (cols doubles) lands at ws[0 .. cols)
int64_t strip_ws_doubles(int32_t n, int32_t cols);
// column sums = the row sums of S for the strip's samples (S symmetric), exact integers as doubles
hipError_t launch_strip_col_sums(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int32_t cols, double* ws,
                                 hipStream_t stream);
// y[jj] = sum_i B(col0 + jj, i) v[i],  B(j, i) = ((S(i, jj) - means[j]) - means[i]) + matrix_mean: row j of the centred
// matrix in the reference's operation order (VariantsPca.scala:216-221), from the strip's column (S is symmetric)
hipError_t launch_strip_matvec(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int32_t col0, int32_t cols,
                               const double* v, const double* means, double matrix_mean, double* ws, hipStream_t stream);
// pcoa_compute_strips: the column sums as exact int64 and as doubles into out_i64[0..cols) / out_f64[0..cols) (any buffers
// on the ws's device, e.g. the lead's N-vectors at the owner's columns)
hipError_t launch_strip_col_sums_to(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int32_t cols, double* ws,
                                    int64_t* out_i64, double* out_f64, hipStream_t stream);
// launch_strip_matvec with the piece written to y_out[0..cols) (a device pointer the ws's device can write: same device or
// peer-mapped) instead of ws[0..cols); bit-identical values
hipError_t launch_strip_matvec_to(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int32_t col0, int32_t cols,
                                  const double* v, const double* means, double matrix_mean, double* ws, double* y_out,
                                  hipStream_t stream);

// pcoa_project (center.hip): rows [0, n_ref) of a strip, columns = the samples to place.  colsum[jj] = sum_{i < n_ref} S(i, jj)
// (launch_strip_col_sums with n = n_ref), means / matrix_mean = the reference's centring, u = k components [k][n_ref], lam = their
// k eigenvalues (device).  out[c * cols + jj] = (sum_j b(jj, j) u_c[j]) / lam[c], b in the reference's operation order.
// k must be 1, 2, 4 or 8 (project_chunk picks the chunk); ws: project_ws_doubles(n_ref, cols, k) doubles.
int64_t project_ws_doubles(int32_t n_ref, int32_t cols, int32_t k);
int project_chunk(int32_t remaining);
hipError_t launch_project(const int32_t* s32, const int64_t* s64_or_null, int32_t n_ref, int32_t cols, const double* colsum,
                          const double* means, double matrix_mean, const double* u, int32_t k, const double* lam, double* ws,
                          double* out, hipStream_t stream);

// ---- symmetric eigensolver (eig.hip) ----------------------------------------------------------
// launch forms of the dense solver (pcoa_timings.eig_dense_form, include/pcoa.h)
constexpr int32_t EIG_FORM_FUSED = 1;              // tridiagonalisation: fused step, one launch per column
constexpr int32_t EIG_FORM_FUSED_BIG_LDS = 2;      // ... with more than 64 KiB of dynamic LDS
constexpr int32_t EIG_FORM_TWO_KERNEL = 4;         // tridiagonalisation: tridiag_hw_kernel + tridiag_update_kernel per column
constexpr int32_t EIG_FORM_BISECT_LDS = 8;         // bisection reads d / e^2 from LDS
constexpr int32_t EIG_FORM_INVIT_LDS = 16;         // inverse iteration keeps its LU factors in LDS
constexpr int32_t EIG_FORM_INVIT_PER_VECTOR = 32;  // inverse iteration: one workgroup per vector
constexpr int32_t EIG_FORM_WY_BACKTRANSFORM = 64;  // blocked compact-WY back-transform
struct EigWorkspace {
  double* a;        // [n][n] in: symmetric matrix B; out: reflector vectors in rows (row k, cols k+1..n-1)
  double* d;        // [n]   diagonal of T
  double* e;        // [n]   off-diagonal of T (n-1 used)
  double* tau;      // [n]   reflector scalars (n-2 used)
  double* q;        // [n]   A22 * v  (raw matvec of the current step)
  double* w;        // [n]   rank-2 update vector of the previous step
  double* lam;      // [2*kmax] candidate eigenvalues (k largest then k smallest)
  double* z;        // [kmax][n] eigenvectors of T, then of A (column c at z + c*n)
  double* scratch;  // [6][n] LU factors for inverse iteration
  int32_t* iscratch;// [2n + 64] pivots / eigenvalue indices
  double* wy;       // blocked back-transform: wy_workspace_doubles(n, kmax) doubles, or nullptr (serial form)
  double* host_rec = nullptr;   // pinned host memory for the Lanczos check record (host_rec_cap doubles), or nullptr
  size_t host_rec_cap = 0;
  // Implicit form of B for the Lanczos path: B(i,j) = ((S(i,j) - rowmean(i)) - colmean(j)) + mean is evaluated on
  // the fly from the integer S (the same expression, operation order and rounding as center_kernel, so the matvec sees
  // bit-identical entries) and the N x N fp64 matrix is never written.  a == nullptr then.
  const int32_t* s32;     // [n][n]
  const int64_t* s64;     // [n][n] or nullptr
  const double* colmean;  // [n] rowSums(j) / N
  const double* stats;    // stats[1] = matrixMean
  // large N: workspace of the symmetric mat-vec that reads only the upper triangle of S (symv_sym_workspace_doubles(n)
  // doubles: 1024 row sums + 1024 column sums per upper-triangular 1024 x 1024 tile), or nullptr: one wave per row
  double* sym_part = nullptr;
  bool band_only = false;   // PCOA_FLAG_EIG_BAND: skip the single-vector iteration (eigenvalues of multiplicity > 1)
  // A similarity measure other than the shared count (pcoa_set_similarity, measure.hip): the implicit forms evaluate
  // K(i, j) from S(i, j) and the two samples' diagonal entries before they centre it; colmean / stats are then K's.
  int measure = 0;                 // PCOA_SIMILARITY_*
  const int64_t* diag = nullptr;   // [n] d_i = S(i, i), the total entry
  const double* qcos = nullptr;    // [n] cosine: q_i = d_i > 0 ? 1 / sqrt(d_i) : 0  (q is the tridiagonalisation's)
  // The pairwise-complete similarity (pcoa_set_call_companion, complete.hip): the implicit forms evaluate K(i, j) from S(i, j),
  // the companion's Q(i, j) and the two samples' called counts before they centre it; colmean / stats are then K's.
  const int32_t* comp_q32 = nullptr;   // [n][n] the companion's finalized int32 S, or nullptr: no companion bound
  const int64_t* comp_c = nullptr;     // [n] c_i = V - Q(i, i)
  int64_t comp_v = 0;                  // V, the variants fed
};
size_t symv_sym_workspace_doubles(int32_t n);
// exact row sums of a finalized (symmetric) int32 S from its upper-triangular tiles: half the bytes of launch_center's row
// pass; sym_part = the mat-vec's workspace (symv_sym_workspace_doubles(n) doubles), n % 4 == 0
hipError_t launch_row_sums_sym(const int32_t* s32, int32_t n, double* sym_part, double* row_sums, int64_t* row_sums_i64,
                               hipStream_t stream);
void launch_centred_matvec(const EigWorkspace& ws, int32_t n, const double* x, double* y, hipStream_t stream);  // one y = B x (test hook)
// y_i = the partials of the upper-triangle form (symv_sym_workspace_doubles(n) doubles, the layout of symv_sym_tiles_kernel)
// added in symv_sym_gather_kernel's fixed order
hipError_t launch_symv_sym_gather(const double* sym_part, int32_t n, double* y, hipStream_t stream);

// ---- similarity measures evaluated on the fly from S (measure.hip; pcoa_set_similarity) ---------------------------------
// kind = PCOA_SIMILARITY_JACCARD | _COSINE.  With s = the total entry (s32 + s64 where there is one), d = its diagonal:
//   Jaccard  U = d_i + d_j - s (int64);  K = U > 0 ? (double)s / (double)U : 0.0
//   cosine   q_i = d_i > 0 ? 1.0 / sqrt((double)d_i) : 0.0;  K = ((double)s * q_i) * q_j
//   centred  B = ((K - r_i / N) - r_j / N) + mm,  r = the row sums of K,  mm = (sum_i r_i) / N / N    (no contraction)
// diag [n] (both kinds) and q [n] (cosine; may be NULL for Jaccard) from the current S
hipError_t launch_measure_diag(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int kind, int64_t* diag, double* q,
                               hipStream_t stream);
// row_sums[i] = sum_j K(i, j), one wave per row, added in row_dot's order (ones: n doubles the call fills with 1.0)
hipError_t launch_measure_row_sums(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int kind, const int64_t* diag,
                                   const double* q, double* ones, double* row_sums, hipStream_t stream);
// the same from the upper-triangular tiles of an int32 S, n % 4 == 0 (sym_part: symv_sym_workspace_doubles(n) doubles): the
// tiles' partials in symv_sym_gather_kernel's order
hipError_t launch_measure_row_sums_sym(const int32_t* s32, int32_t n, int kind, const int64_t* diag, const double* q,
                                       double* ones, double* sym_part, double* row_sums, hipStream_t stream);
// stats[0] = sum_i row_sums[i] (one workgroup: thread t adds i = t, t + 256, .. in order, then the 64 lanes of a wave by
// halving strides, then the four waves left to right), stats[1] = stats[0] / N / N, nz[0] = #{i : row_sums[i] > 0}
hipError_t launch_measure_stats(const double* row_sums, int32_t n, double* stats, int32_t* nz, hipStream_t stream);
// b = B, [n][n] fp64 (cm = row_sums / N: launch_col_means)
hipError_t launch_measure_center(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int kind, const int64_t* diag,
                                 const double* q, const double* cm, const double* stats, double* b, hipStream_t stream);
// y = B x through the implicit forms: upper-triangular tiles when ws.sym_part is set (int32 S, n % 4 == 0), else one wave per row
hipError_t launch_measure_symv(const EigWorkspace& ws, int32_t n, const double* x, double* y, hipStream_t stream);

// ---- the pairwise-complete similarity, evaluated on the fly from S and the companion's Q (complete.hip; pcoa_set_call_companion)
//   c_i = V - Q(i, i);  M = c_i + c_j - V + Q(i, j) (int64);  K = M > 0 ? (double)s / (double)M : 0.0;  centred as above
// s = the total entry (s32 + s64 where there is one); q32 = the companion's finalized int32 matrix (it has no int64 part)
// c[i] = V - Q(i, i) for the n samples; flag[0] = 1 if some Q(i, i) > V, else 0
hipError_t launch_complete_diag(const int32_t* q32, int32_t n, int64_t v, int64_t* c, int32_t* flag, hipStream_t stream);
// row_sums[i] = sum_j K(i, j), one wave per row, added in row_dot's order (ones: n doubles the call fills with 1.0)
hipError_t launch_complete_row_sums(const int32_t* s32, const int64_t* s64_or_null, const int32_t* q32, int32_t n, const int64_t* c,
                                    int64_t v, double* ones, double* row_sums, hipStream_t stream);
// the same from the upper-triangular tiles of the two int32 matrices, n % 4 == 0, in symv_sym_gather_kernel's order
hipError_t launch_complete_row_sums_sym(const int32_t* s32, const int32_t* q32, int32_t n, const int64_t* c, int64_t v, double* ones,
                                        double* sym_part, double* row_sums, hipStream_t stream);
// b = B, [n][n] fp64 (cm = row_sums / N: launch_col_means; stats: launch_measure_stats)
hipError_t launch_complete_center(const int32_t* s32, const int64_t* s64_or_null, const int32_t* q32, int32_t n, const int64_t* c,
                                  int64_t v, const double* cm, const double* stats, double* b, hipStream_t stream);
// y = B x through the implicit forms (ws.comp_*): upper-triangular tiles when ws.sym_part is set, else one wave per row
hipError_t launch_complete_symv(const EigWorkspace& ws, int32_t n, const double* x, double* y, hipStream_t stream);
// PLINK .bed rows -> carrier bitsets (bit for bit launch_plink_bed_to_bits) and missing-call bitsets (code 01), one read
hipError_t launch_plink_bed_to_bits_pair(const uint8_t* bed, int64_t row_bytes, int64_t nv, int32_t n, int64_t words, int ref_a1,
                                         uint32_t* bits, uint32_t* miss, hipStream_t stream);
// form (optional): the launcher ORs in the EIG_FORM_* bits (pcoa.h, pcoa_timings.eig_dense_form) of the form it launched
hipError_t launch_tridiagonalize(const EigWorkspace& ws, int32_t n, hipStream_t stream, int32_t* form = nullptr);
// eigenvalues with ascending indices idx[0..count) of T -> lam_out[0..count) (device)
hipError_t launch_bisect(const EigWorkspace& ws, int32_t n, const int32_t* idx_host, int32_t count,
                         double* lam_out_dev, hipStream_t stream, int32_t* form = nullptr);
// eigenvectors of T for lam_sel[0..k) (host values) -> ws.z
hipError_t launch_inverse_iteration(const EigWorkspace& ws, int32_t n, const double* lam_sel_host, int32_t k,
                                    hipStream_t stream, int32_t* form = nullptr);
// the same with lam_sel already in ws.lam[0..k) on the device (one workgroup, vectors in sequence)
hipError_t launch_inverse_iteration_dev(const EigWorkspace& ws, int32_t n, int32_t k, hipStream_t stream);
// ws.z <- Q * ws.z (if apply_reflectors), normalise, sign-normalise (optional); out_dev[c*n + i] column-major
size_t wy_workspace_doubles(int32_t n, int32_t k);
hipError_t launch_backtransform(const EigWorkspace& ws, int32_t n, int32_t k, int sign_normalize,
                                int apply_reflectors, double* out_dev, hipStream_t stream, int32_t* form = nullptr);

// ---- Lanczos fast path (eig_lanczos.hip) ------------------------------------------------------
size_t lanczos_workspace_doubles(int32_t n, int32_t k, int32_t mmax);
// mv (optional): the caller's y = B v on device vectors (return 0); nullptr = the engine's own mat-vec on ws
typedef std::function<int(const double*, double*)> LanczosMatvec;
// band_steps_out (optional): basis vectors the band-Lanczos fallback built (0 = the single-vector iteration sufficed)
hipError_t lanczos_topk(const EigWorkspace& ws, double* lz, int32_t n, int32_t k, int32_t mmax, double tol,
                        double* lam_sel_host, int* converged, int* steps_out, hipStream_t stream,
                        const LanczosMatvec* mv = nullptr, int* band_steps_out = nullptr);

}  // namespace pcoa

#endif  // PCOA_INTERNAL_H_
