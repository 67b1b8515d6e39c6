// capi_grm_dense.hip -- reading K out (pcoa_grm_block): a rectangle of the matrix a GRM ctx decomposes, and of the
// pair counts, as a dense fp64 product of the 2-bit store with itself on the matrix cores (grm_dense.hip).  One launch per
// segment of the store, in order, continuing from the output; then one division per entry.  Nothing here writes the store, and
// the counts and weights are the resident ones of capi_grm.hip.
#include <algorithm>
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

}  // namespace

extern "C" {

int pcoa_grm_block(pcoa_ctx* c, int32_t row0, int32_t rows, int32_t col0, int32_t cols, int32_t divisor, double* out_k,
                   int32_t* out_pairs, int is_device_ptr) {
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_grm_block: ctx is NULL");
  const std::string rect = "rows [" + std::to_string(row0) + ", " + std::to_string((int64_t)row0 + rows) + ") x columns [" +
                           std::to_string(col0) + ", " + std::to_string((int64_t)col0 + cols) + ")";
  if (rows < 1 || cols < 1) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_block: " + rect + ": rows and cols must be at least 1");
  if (row0 < 0 || col0 < 0 || rows > c->n - row0 || cols > c->n - col0)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_block: " + rect + " is not inside [0, " + std::to_string(c->n) + ")^2");
  if (divisor != PCOA_GRM_DIVISOR_USED && divisor != PCOA_GRM_DIVISOR_PAIRWISE)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_block: divisor = " + std::to_string(divisor) +
                                             " is neither PCOA_GRM_DIVISOR_USED (0) nor PCOA_GRM_DIVISOR_PAIRWISE (1)");
  if (!out_k && !out_pairs) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_block: out_k and out_pairs are both NULL");
  if (!c->is_grm)
    return fail(c, PCOA_ERR_STATE, std::string("pcoa_grm_block: not a GRM ctx (pcoa_create_grm) but ") + kind_of(c) +
                                       ": there is no genotype store to build K from");
  if (c->is_grm_study)
    return fail(c, PCOA_ERR_STATE, "pcoa_grm_block: a GRM study ctx (pcoa_create_grm_study) holds the genotypes of study samples and "
                                   "no weights of its own; pass it to pcoa_grm_project beside the panel's ctx");
  CHECK_CTX(c);
  int rc = check_device_flags(c);
  if (rc != PCOA_OK) return rc;
  GrmParams g;
  int64_t used = 0;
  if ((rc = grm_resident_params(c, &g, &used)) != PCOA_OK) return rc;
  if (used == 0)
    return fail(c, PCOA_ERR_STATE, "pcoa_grm_block: none of the " + std::to_string(c->op_variants) +
                                       " variants in the store is used (polymorphic, called, at or above min_maf): K is undefined");
  if (used >= ((int64_t)1 << 31))
    return fail(c, PCOA_ERR_STATE, "pcoa_grm_block: M' = " + std::to_string(used) + " used variants do not fit the int32 pair counts");

  // the accumulators: the caller's device memory, or the ctx's block buffer ([total] doubles | [total] int32)
  const int64_t total = (int64_t)rows * cols;
  const bool want_k = out_k != nullptr;
  const bool want_n = out_pairs != nullptr || (want_k && divisor == PCOA_GRM_DIVISOR_PAIRWISE);
  const bool own_k = want_k && !is_device_ptr, own_n = want_n && !(is_device_ptr && out_pairs);
  if (own_k || own_n) {
    if ((rc = ensure(c, &c->grm_blk, &c->grm_blk_cap, (own_k ? total : 0) + (own_n ? (total + 1) / 2 : 0))) != PCOA_OK) return rc;
  }
  double* const k_dev = !want_k ? nullptr : own_k ? c->grm_blk : out_k;
  int32_t* const n_dev = !want_n ? nullptr : own_n ? reinterpret_cast<int32_t*>(c->grm_blk + (own_k ? total : 0)) : out_pairs;
  {
    ScopedTimer t(c, T_GRM_BLOCK);
    int64_t seg_row0 = 0;
    int first = 1;
    for (const auto& s : c->op_segs) {
      if (s.rows <= 0) continue;
      HIP_TRY(c, launch_grm_dense(s.p, (int32_t)s.rows, c->n, g.mu + seg_row0, g.d + seg_row0, g.used + seg_row0, row0, rows, col0, cols,
                                  first, k_dev, n_dev, c->stream));
      seg_row0 += s.rows;
      first = 0;
    }
    if (want_k) HIP_TRY(c, launch_grm_dense_finish(k_dev, n_dev, total, divisor, used, c->stream));
  }
  if (own_k) HIP_TRY(c, hipMemcpyAsync(out_k, k_dev, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
  if (out_pairs && own_n) HIP_TRY(c, hipMemcpyAsync(out_pairs, n_dev, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->grm_block_calls += 1;
  c->grm_block_flops += 2.0 * (double)rows * (double)cols * (double)c->op_variants * (double)((want_k ? 1 : 0) + (want_n ? 1 : 0));
  return PCOA_OK;
}

int pcoa_get_grm_block_stats(pcoa_ctx* c, pcoa_grm_block_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_grm_block_stats full;
  std::memset(&full, 0, sizeof(full));
  full.grm_block_seconds = c->tsec[T_GRM_BLOCK];
  full.grm_block_calls = c->grm_block_calls;
  full.grm_block_flops = c->grm_block_flops;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
