// capi_grm_king.hip -- pcoa_grm_king_block / pcoa_grm_king_pairs: the KING-robust kinship screen on the resident 2-bit store of a
// GRM ctx (the rule is stated at the block of pcoa.h, the kernels are grm_king.hip's, variants_pca.py's
// grm_king_rule / grm_king_pairs_rule are the numpy statement).  The block call reads a rectangle of the three counts out; the
// pairs call walks the upper triangle in bands of band_rows rows as pcoa_grm_pairs does: the count kernel's launches (one per
// segment of the store) fill the band's three int32 arrays in the ctx's block buffer, the screen counts, scans and writes them,
// and the next band reuses the buffer behind it on the same stream.  The running pair count stays on the device, so the only
// read-back is n_found at the end.  Arguments are validated on the host before anything touches a device; every buffer is
// allocated before the first launch and the call's own are freed before it returns.  Nothing here writes the store.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace {

const char* kind_of(const pcoa_ctx* c) {
  if (c->is_strip) return "a strip owner (pcoa_create_strip)";
  if (c->is_operator) return "an operator ctx (pcoa_create_operator)";
  return "a full engine (pcoa_create)";
}

constexpr int32_t kGrmKingDefaultBandRows = 1024;

// the host checks the two calls share, in this order: rows_kind, then the ctx's kind
int check_rows_kind(pcoa_ctx* c, const char* call, int32_t rows_kind) {
  if (rows_kind != PCOA_GRM_ROWS_ALL && rows_kind != PCOA_GRM_ROWS_USED)
    return fail(c, PCOA_ERR_INVALID_ARG, std::string(call) + ": rows_kind = " + std::to_string(rows_kind) +
                                             " is neither PCOA_GRM_ROWS_ALL (0) nor PCOA_GRM_ROWS_USED (1)");
  return PCOA_OK;
}

int check_store(pcoa_ctx* c, const char* call, int32_t rows_kind) {
  if (!c->is_grm)
    return fail(c, PCOA_ERR_STATE, std::string(call) + ": not a GRM ctx (pcoa_create_grm, pcoa_create_grm_study) but " + kind_of(c) +
                                       ": there is no genotype store to count classes in");
  if (rows_kind == PCOA_GRM_ROWS_USED && c->is_grm_study)
    return fail(c, PCOA_ERR_STATE, std::string(call) + ": PCOA_GRM_ROWS_USED on a GRM study ctx (pcoa_create_grm_study), which has no "
                                                       "used_v of its own; PCOA_GRM_ROWS_ALL counts every row of its store");
  return PCOA_OK;
}

// the counted rows and, under PCOA_GRM_ROWS_USED, used_v of the resident weights (NULL: every row counts)
int counted_rows(pcoa_ctx* c, const char* call, int32_t rows_kind, const int32_t** used_out, int64_t* counted_out) {
  const int32_t* used = nullptr;
  int64_t counted = c->op_variants;
  if (rows_kind == PCOA_GRM_ROWS_USED && c->op_variants > 0) {   // (an empty store has no weights to compute)
    const int rc = grm_resident_weights(c);
    if (rc != PCOA_OK) return rc;
    used = grm_used_rows(c);
    counted = c->grm_used;
  }
  if (counted == 0)
    return fail(c, PCOA_ERR_STATE, std::string(call) + ": none of the " + std::to_string(c->op_variants) + " variants in the store is " +
                                       (rows_kind == PCOA_GRM_ROWS_USED ? "used (polymorphic, called, at or above min_maf, passing the "
                                                                          "filters and the LD mask)"
                                                                        : "there to count") +
                                       ": the kinship is undefined");
  if (counted >= ((int64_t)1 << 30))
    return fail(c, PCOA_ERR_STATE, std::string(call) + ": " + std::to_string(counted) +
                                       " counted rows: het_sum <= 2 V does not fit the int32 counts from 2^30 rows on");
  *used_out = used;
  *counted_out = counted;
  return PCOA_OK;
}

// int8 multiply-adds the count kernel issues for one rectangle: whole 64 x 64 tiles, rows rounded up to the k-step per segment
double king_macs(const pcoa_ctx* c, int32_t row0, int32_t rows, int32_t col0, int32_t cols) {
  const double tr = (double)((row0 + rows - 1) / 64 - row0 / 64 + 1), tc = (double)((col0 + cols - 1) / 64 - col0 / 64 + 1);
  double k = 0;
  for (const auto& s : c->op_segs)
    if (s.rows > 0) k += (double)((s.rows + 31) / 32 * 32);
  return 4.0 * (tr * 64.0) * (tc * 64.0) * k;
}

}  // namespace

extern "C" {

int pcoa_grm_king_block(pcoa_ctx* c, int32_t rows_kind, int32_t row0, int32_t rows, int32_t col0, int32_t cols, int32_t* out_hethet,
                        int32_t* out_ibs0, int32_t* out_het_sum, int is_device_ptr) {
  const char* fn = "pcoa_grm_king_block";
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_block: ctx is NULL");
  const std::string rect = "rows [" + std::to_string(row0) + ", " + std::to_string((int64_t)row0 + rows) + ") x columns [" +
                           std::to_string(col0) + ", " + std::to_string((int64_t)col0 + cols) + ")";
  if (rows < 1 || cols < 1) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_block: " + rect + ": rows and cols must be at least 1");
  if (row0 < 0 || col0 < 0 || rows > c->n - row0 || cols > c->n - col0)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_block: " + rect + " is not inside [0, " + std::to_string(c->n) + ")^2");
  int rc = check_rows_kind(c, fn, rows_kind);
  if (rc != PCOA_OK) return rc;
  if (!out_hethet && !out_ibs0 && !out_het_sum)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_block: out_hethet, out_ibs0 and out_het_sum are all NULL");
  if ((rc = check_store(c, fn, rows_kind)) != PCOA_OK) return rc;
  CHECK_CTX(c);
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  const int32_t* used = nullptr;
  int64_t counted = 0;
  if ((rc = counted_rows(c, fn, rows_kind, &used, &counted)) != PCOA_OK) return rc;

  // the outputs: the caller's device memory, or one [total] int32 array per output in the ctx's block buffer
  const int64_t total = (int64_t)rows * cols;
  int32_t* user[3] = {out_hethet, out_ibs0, out_het_sum};
  int32_t* dev[3] = {out_hethet, out_ibs0, out_het_sum};
  if (!is_device_ptr) {
    int wanted = 0;
    for (int k = 0; k < 3; ++k) wanted += user[k] ? 1 : 0;
    if ((rc = ensure(c, &c->grm_blk, &c->grm_blk_cap, (wanted * total + 1) / 2)) != PCOA_OK) return rc;
    int32_t* base = reinterpret_cast<int32_t*>(c->grm_blk);
    for (int k = 0, at = 0; k < 3; ++k)
      if (user[k]) dev[k] = base + (int64_t)(at++) * total;
  }
  {
    ScopedTimer t(c, T_GRM_KING_COUNTS);
    int64_t seg_row0 = 0;
    int first = 1;
    for (const auto& s : c->op_segs) {
      if (s.rows <= 0) continue;
      HIP_TRY(c, launch_grm_king_counts(s.p, (int32_t)s.rows, c->n, used ? used + seg_row0 : nullptr, row0, rows, col0, cols, first, dev[0],
                                        dev[1], dev[2], c->stream));
      seg_row0 += s.rows;
      first = 0;
    }
  }
  if (!is_device_ptr)
    for (int k = 0; k < 3; ++k)
      if (user[k]) HIP_TRY(c, hipMemcpyAsync(user[k], dev[k], sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->grm_king_block_calls += 1;
  c->grm_king_macs += king_macs(c, row0, rows, col0, cols);
  return PCOA_OK;
}

int pcoa_grm_king_pairs(pcoa_ctx* c, int32_t rows_kind, double min_kinship, int32_t band_rows, pcoa_king_pair* out_pairs,
                        int64_t capacity, int64_t* n_found_out, int64_t* n_rows_out, int64_t* out_het) {
  const char* fn = "pcoa_grm_king_pairs";
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_pairs: ctx is NULL");
  if (!n_found_out) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_pairs: n_found_out is NULL");
  int rc = check_rows_kind(c, fn, rows_kind);
  if (rc != PCOA_OK) return rc;
  if (!std::isfinite(min_kinship) || !(min_kinship > 0.0) || min_kinship > 0.5)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_pairs: min_kinship = " + std::to_string(min_kinship) +
                                             " is not a finite number in (0, 0.5]");
  if (band_rows < 0 || band_rows % 64 != 0)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_pairs: band_rows = " + std::to_string(band_rows) +
                                             " is neither 0 (1,024 rows) nor a positive multiple of 64");
  if (capacity < 0) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_pairs: capacity = " + std::to_string(capacity) + " is negative");
  if (capacity > 0 && !out_pairs)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_king_pairs: out_pairs is NULL with capacity = " + std::to_string(capacity) +
                                             " (capacity 0 is the count-only call)");
  if ((rc = check_store(c, fn, rows_kind)) != PCOA_OK) return rc;
  CHECK_CTX(c);
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  const int32_t* used = nullptr;
  int64_t counted = 0;
  if ((rc = counted_rows(c, fn, rows_kind, &used, &counted)) != PCOA_OK) return rc;

  const int32_t n = c->n;
  const int64_t npad = ((int64_t)n + 63) / 64 * 64;   // a band's columns end here: its pitch npad - c0 is a multiple of 64 int32
  const int32_t band = (int32_t)std::min<int64_t>(band_rows ? band_rows : kGrmKingDefaultBandRows, npad);
  const int64_t most = (int64_t)n * (int64_t)(n - 1) / 2;   // the rule cannot report more pairs than there are
  const int64_t cap_dev = std::min(capacity, most);
  const size_t ntiles_max = (size_t)grm_pairs_tiles(n);

  // the band: three [band][npad] int32 arrays in the buffer pcoa_grm_block grows (each starts on a multiple of 256 bytes)
  const int64_t band_elems = (int64_t)band * npad;
  if ((rc = ensure(c, &c->grm_blk, &c->grm_blk_cap, (3 * band_elems + 1) / 2)) != PCOA_OK) return rc;
  int32_t* const hh_dev = reinterpret_cast<int32_t*>(c->grm_blk);
  int32_t* const ib_dev = hh_dev + band_elems;
  int32_t* const hs_dev = ib_dev + band_elems;
  // the call's own: rowoff [band + 1], the running total and the write pass's entry counter in one int64 block, the counts, h,
  // the pairs
  int64_t* words = nullptr;
  int32_t* cnt = nullptr;
  int64_t* het = nullptr;
  pcoa_king_pair* pairs_dev = nullptr;
  auto release = [&]() {
    dev_free(words);
    dev_free(cnt);
    dev_free(het);
    dev_free(pairs_dev);
    words = nullptr;
    cnt = nullptr;
    het = nullptr;
    pairs_dev = nullptr;
  };
  auto alloc_bail = [&](hipError_t e, const char* what) {
    release();
    return hip_fail(c, e, what);   // hipErrorOutOfMemory comes back as PCOA_ERR_OUT_OF_MEMORY
  };
  hipError_t e;
  if ((e = dev_alloc((void**)&words, sizeof(int64_t) * ((size_t)band + 3), c->device)) != hipSuccess)
    return alloc_bail(e, "the row offsets");
  if ((e = dev_alloc((void**)&cnt, sizeof(int32_t) * (size_t)band * ntiles_max, c->device)) != hipSuccess)
    return alloc_bail(e, "the (row, tile) counts");
  if (out_het && (e = dev_alloc((void**)&het, sizeof(int64_t) * (size_t)n, c->device)) != hipSuccess) return alloc_bail(e, "h");
  if (cap_dev > 0 && (e = dev_alloc((void**)&pairs_dev, sizeof(pcoa_king_pair) * (size_t)cap_dev, c->device)) != hipSuccess)
    return alloc_bail(e, "the pairs");
  int64_t* const rowoff = words;            // band + 1 entries
  int64_t* const total = words + band + 1;  // the pairs of the bands so far
  unsigned long long* const entries_read = (unsigned long long*)(words + band + 2);
  // once a launch is queued the buffers are only freed behind the stream
  auto hip_bail = [&](hipError_t err, const char* what) {
    (void)hipStreamSynchronize(c->stream);
    release();
    return hip_fail(c, err, what);
  };
  if ((e = hipMemsetAsync(total, 0, 2 * sizeof(int64_t), c->stream)) != hipSuccess) return hip_bail(e, "hipMemsetAsync");
  int64_t bands = 0, count_entries = 0;
  double macs = 0;
  for (int32_t r0 = 0; r0 < n; r0 += band) {
    const int32_t nrows = std::min(band, n - r0);
    const int32_t c0 = r0 / 64 * 64;
    const int32_t pitch = (int32_t)(npad - c0);
    {
      ScopedTimer t(c, T_GRM_KING_COUNTS);
      int64_t seg_row0 = 0;
      int first = 1;
      for (const auto& s : c->op_segs) {
        if (s.rows <= 0) continue;
        if ((e = launch_grm_king_counts(s.p, (int32_t)s.rows, n, used ? used + seg_row0 : nullptr, r0, nrows, c0, pitch, first, hh_dev,
                                        ib_dev, hs_dev, c->stream)) != hipSuccess)
          return hip_bail(e, "grm_king_counts_kernel");
        seg_row0 += s.rows;
        first = 0;
      }
    }
    {
      ScopedTimer t(c, T_GRM_KING_SCREEN);
      if ((e = launch_grm_king_screen_count(hh_dev, ib_dev, hs_dev, pitch, r0, nrows, c0, n, min_kinship, cnt, het, c->stream)) !=
          hipSuccess)
        return hip_bail(e, "grm_king_screen_count_kernel");
      if ((e = launch_grm_pairs_scan(cnt, nrows, grm_pairs_tiles(n - c0), rowoff, total, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_pairs scan kernels");
      if (cap_dev > 0 && (e = launch_grm_king_screen_write(hh_dev, ib_dev, hs_dev, pitch, r0, nrows, c0, n, min_kinship, cnt, rowoff,
                                                           cap_dev, pairs_dev, entries_read, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_king_screen_write_kernel");
    }
    bands += 1;
    count_entries += grm_pairs_count_pass_entries(r0, nrows, c0, n);
    macs += king_macs(c, r0, nrows, c0, pitch);
  }
  // n_found and the entry counter land in the ctx's pinned words
  if ((e = hipMemcpyAsync(&c->hw->coll[0], total, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(n_found)");
  if ((e = hipMemcpyAsync(&c->hw->coll[1], entries_read, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(entries read)");
  if (out_het && (e = hipMemcpyAsync(out_het, het, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(h)");
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  const int64_t n_found = c->hw->coll[0];
  const int64_t reread = c->hw->coll[1];
  if (n_found < 0 || n_found > most) {   // cannot happen; never copy by a count that is not one
    release();
    return fail(c, PCOA_ERR_HIP, "pcoa_grm_king_pairs: the scan returned " + std::to_string(n_found) + " pairs of at most " +
                                     std::to_string(most));
  }
  const int64_t written = std::min(n_found, cap_dev);
  if (written > 0) {
    if ((e = hipMemcpyAsync(out_pairs, pairs_dev, sizeof(pcoa_king_pair) * (size_t)written, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
      return hip_bail(e, "hipMemcpyAsync(pairs)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  }
  release();
  c->grm_king_calls += 1;
  c->grm_king_bands += bands;
  c->grm_king_macs += macs;
  c->grm_king_bytes += 3 * (int64_t)sizeof(int32_t) * (count_entries + reread);
  *n_found_out = n_found;
  if (n_rows_out) *n_rows_out = counted;
  return PCOA_OK;
}

int pcoa_get_grm_king_stats(pcoa_ctx* c, pcoa_grm_king_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_grm_king_stats full;
  std::memset(&full, 0, sizeof(full));
  full.grm_king_seconds = c->tsec[T_GRM_KING_COUNTS] + c->tsec[T_GRM_KING_SCREEN];
  full.grm_king_screen_seconds = c->tsec[T_GRM_KING_SCREEN];
  full.grm_king_calls = c->grm_king_calls;
  full.grm_king_bands = c->grm_king_bands;
  full.grm_king_macs = c->grm_king_macs;
  full.grm_king_bytes = c->grm_king_bytes;
  full.grm_king_block_calls = c->grm_king_block_calls;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
