// capi_grm_pairs.hip -- pcoa_grm_pairs: the relatedness cut-off on the K of a GRM ctx.  The rule
// (grm_pairs.hip compares on the device; variants_pca.py's grm_pairs_rule is the numpy statement): the pair (i, j), i < j, is
// reported iff K(i, j) >= cutoff, K(i, j) the bits pcoa_grm_block returns.  The upper triangle is walked in bands of band_rows
// rows: pcoa_grm_block's own launches (one per segment of the store, then the division) fill the band in the ctx's block
// buffer, the screen counts, scans and writes it, and the next band reuses the buffer behind it on the same stream.  The running
// pair count stays on the device, so the only read-back is n_found at the end.  Arguments are validated on the host before
// anything touches a device; every buffer is allocated before the first launch and the call's own are freed before it returns.
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

constexpr int32_t kGrmPairsDefaultBandRows = 1024;

}  // namespace

extern "C" {

int pcoa_grm_pairs(pcoa_ctx* c, double cutoff, int32_t divisor, int32_t band_rows, pcoa_grm_pair* out_pairs, int64_t capacity,
                   int64_t* n_found_out, double* out_diag) {
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_grm_pairs: ctx is NULL");
  if (!n_found_out) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_pairs: n_found_out is NULL");
  if (!std::isfinite(cutoff))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_pairs: cutoff = " + std::to_string(cutoff) + " is not a finite number");
  if (divisor != PCOA_GRM_DIVISOR_USED && divisor != PCOA_GRM_DIVISOR_PAIRWISE)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_pairs: divisor = " + std::to_string(divisor) +
                                             " is neither PCOA_GRM_DIVISOR_USED (0) nor PCOA_GRM_DIVISOR_PAIRWISE (1)");
  if (band_rows < 0 || band_rows % 64 != 0)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_pairs: band_rows = " + std::to_string(band_rows) +
                                             " is neither 0 (1,024 rows) nor a positive multiple of 64");
  if (capacity < 0) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_pairs: capacity = " + std::to_string(capacity) + " is negative");
  if (capacity > 0 && !out_pairs)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_pairs: out_pairs is NULL with capacity = " + std::to_string(capacity) +
                                             " (capacity 0 is the count-only call)");
  if (!c->is_grm)
    return fail(c, PCOA_ERR_STATE, std::string("pcoa_grm_pairs: not a GRM ctx (pcoa_create_grm) but ") + kind_of(c) +
                                       ": there is no genotype store to build K from");
  if (c->is_grm_study)
    return fail(c, PCOA_ERR_STATE, "pcoa_grm_pairs: a GRM study ctx (pcoa_create_grm_study) holds the genotypes of study samples and "
                                   "no weights of its own; pass it to pcoa_grm_project beside the panel's ctx");
  CHECK_CTX(c);
  int rc = check_device_flags(c);
  if (rc != PCOA_OK) return rc;
  GrmParams g;
  int64_t used = 0;
  if ((rc = grm_resident_params(c, &g, &used)) != PCOA_OK) return rc;
  if (used == 0)
    return fail(c, PCOA_ERR_STATE, "pcoa_grm_pairs: none of the " + std::to_string(c->op_variants) +
                                       " variants in the store is used (polymorphic, called, at or above min_maf): K is undefined");
  if (used >= ((int64_t)1 << 31))
    return fail(c, PCOA_ERR_STATE, "pcoa_grm_pairs: M' = " + std::to_string(used) + " used variants do not fit the int32 pair counts");

  const int32_t n = c->n;
  const int64_t npad = ((int64_t)n + 63) / 64 * 64;   // a band's columns end here: its pitch npad - c0 is a multiple of 64 doubles
  const int32_t band = (int32_t)std::min<int64_t>(band_rows ? band_rows : kGrmPairsDefaultBandRows, npad);
  const bool pairwise = divisor == PCOA_GRM_DIVISOR_PAIRWISE;
  const int64_t most = (int64_t)n * (int64_t)(n - 1) / 2;   // the rule cannot report more pairs than there are
  const int64_t cap_dev = std::min(capacity, most);
  const size_t ntiles_max = (size_t)grm_pairs_tiles(n);

  // the band: [band][npad] doubles | [band][npad] int32, in the buffer pcoa_grm_block grows
  const int64_t band_elems = (int64_t)band * npad;
  if ((rc = ensure(c, &c->grm_blk, &c->grm_blk_cap, band_elems + (pairwise ? (band_elems + 1) / 2 : 0))) != PCOA_OK) return rc;
  double* const k_dev = c->grm_blk;
  int32_t* const n_dev = pairwise ? reinterpret_cast<int32_t*>(c->grm_blk + band_elems) : nullptr;
  // the call's own: rowoff [band + 1], the running total and the write pass's entry counter in one int64 block, the counts,
  // the diagonal, the pairs
  int64_t* words = nullptr;
  int32_t* cnt = nullptr;
  double* diag = nullptr;
  pcoa_grm_pair* pairs_dev = nullptr;
  auto release = [&]() {
    dev_free(words);
    dev_free(cnt);
    dev_free(diag);
    dev_free(pairs_dev);
    words = nullptr;
    cnt = nullptr;
    diag = nullptr;
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
  if (out_diag && (e = dev_alloc((void**)&diag, sizeof(double) * (size_t)n, c->device)) != hipSuccess)
    return alloc_bail(e, "the diagonal");
  if (cap_dev > 0 && (e = dev_alloc((void**)&pairs_dev, sizeof(pcoa_grm_pair) * (size_t)cap_dev, c->device)) != hipSuccess)
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
  double flops = 0;
  for (int32_t r0 = 0; r0 < n; r0 += band) {
    const int32_t nrows = std::min(band, n - r0);
    const int32_t c0 = r0 / 64 * 64;
    const int32_t pitch = (int32_t)(npad - c0);
    {
      ScopedTimer t(c, T_GRM_PAIRS_DENSE);
      int64_t seg_row0 = 0;
      int first = 1;
      for (const auto& s : c->op_segs) {
        if (s.rows <= 0) continue;
        if ((e = launch_grm_dense(s.p, (int32_t)s.rows, n, g.mu + seg_row0, g.d + seg_row0, g.used + seg_row0, r0, nrows, c0, pitch,
                                  first, k_dev, n_dev, c->stream)) != hipSuccess)
          return hip_bail(e, "grm_dense_kernel");
        seg_row0 += s.rows;
        first = 0;
      }
      if ((e = launch_grm_dense_finish(k_dev, n_dev, (int64_t)nrows * pitch, divisor, used, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_dense_finish_kernel");
    }
    {
      ScopedTimer t(c, T_GRM_PAIRS_SCREEN);
      if ((e = launch_grm_pairs_count(k_dev, pitch, r0, nrows, c0, n, cutoff, cnt, diag, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_pairs_count_kernel");
      if ((e = launch_grm_pairs_scan(cnt, nrows, grm_pairs_tiles(n - c0), rowoff, total, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_pairs scan kernels");
      if (cap_dev > 0 && (e = launch_grm_pairs_write(k_dev, n_dev, pitch, r0, nrows, c0, n, cutoff, used, cnt, rowoff, cap_dev, pairs_dev,
                                                     entries_read, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_pairs_write_kernel");
    }
    bands += 1;
    count_entries += grm_pairs_count_pass_entries(r0, nrows, c0, n);
    flops += 2.0 * (double)nrows * (double)pitch * (double)c->op_variants * (pairwise ? 2.0 : 1.0);
  }
  // n_found and the entry counter land in the ctx's pinned words
  if ((e = hipMemcpyAsync(&c->hw->coll[0], total, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(n_found)");
  if ((e = hipMemcpyAsync(&c->hw->coll[1], entries_read, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(entries read)");
  if (out_diag && (e = hipMemcpyAsync(out_diag, diag, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(diag)");
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  const int64_t n_found = c->hw->coll[0];
  const int64_t reread = c->hw->coll[1];
  if (n_found < 0 || n_found > most) {   // cannot happen; never copy by a count that is not one
    release();
    return fail(c, PCOA_ERR_HIP, "pcoa_grm_pairs: the scan returned " + std::to_string(n_found) + " pairs of at most " + std::to_string(most));
  }
  const int64_t written = std::min(n_found, cap_dev);
  if (written > 0) {
    if ((e = hipMemcpyAsync(out_pairs, pairs_dev, sizeof(pcoa_grm_pair) * (size_t)written, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
      return hip_bail(e, "hipMemcpyAsync(pairs)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  }
  release();
  c->grm_pairs_calls += 1;
  c->grm_pairs_bands += bands;
  c->grm_pairs_flops += flops;
  c->grm_pairs_bytes += (int64_t)sizeof(double) * count_entries + (int64_t)(sizeof(double) + (pairwise ? sizeof(int32_t) : 0)) * reread;
  *n_found_out = n_found;
  return PCOA_OK;
}

int pcoa_get_grm_pairs_stats(pcoa_ctx* c, pcoa_grm_pairs_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_grm_pairs_stats full;
  std::memset(&full, 0, sizeof(full));
  full.grm_pairs_seconds = c->tsec[T_GRM_PAIRS_DENSE] + c->tsec[T_GRM_PAIRS_SCREEN];
  full.grm_pairs_screen_seconds = c->tsec[T_GRM_PAIRS_SCREEN];
  full.grm_pairs_calls = c->grm_pairs_calls;
  full.grm_pairs_bands = c->grm_pairs_bands;
  full.grm_pairs_flops = c->grm_pairs_flops;
  full.grm_pairs_bytes = c->grm_pairs_bytes;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
