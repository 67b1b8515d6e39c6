// capi_grm_subset.hip -- pcoa_create_grm_subset: a new GRM ctx whose store is another's with the removed samples' columns taken
// out (the kernel is grm_subset.hip).  A GRM ctx keeps 2 bits per genotype and nothing else, so the reduced
// cohort's engine is one gather over the store; its counts, weights and everything behind them are then computed from its own
// columns like any fed engine's.  The kept index set is validated on the host before anything touches a device; the new engine
// comes from pcoa_create_grm's / pcoa_create_grm_study's own path, all of its segments are allocated before the first row moves
// (store_grow), and the gathers run on SRC's stream -- behind its appends -- one launch per intersection of a source segment
// with a result segment (store_append cuts a source segment's rows at the result's segment boundaries).  Also here:
// pcoa_grm_rows, the store's rows read back as .bed rows.
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

int pcoa_create_grm_subset(pcoa_ctx** out, pcoa_ctx* src, const int32_t* keep, int32_t n_keep, int32_t kind) {
  if (!out) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_create_grm_subset: out is NULL");
  *out = nullptr;
  if (!src) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_create_grm_subset: src ctx is NULL");
  if (!src->is_grm)
    return fail(src, PCOA_ERR_STATE, std::string("pcoa_create_grm_subset: src is not a GRM ctx (pcoa_create_grm, pcoa_create_grm_study) but ") +
                                         kind_of(src) + ": there is no genotype store to take columns from");
  if (kind != PCOA_GRM_SUBSET_PANEL && kind != PCOA_GRM_SUBSET_STUDY)
    return fail(src, PCOA_ERR_INVALID_ARG, "pcoa_create_grm_subset: kind = " + std::to_string(kind) +
                                               " is neither PCOA_GRM_SUBSET_PANEL (0) nor PCOA_GRM_SUBSET_STUDY (1)");
  const int32_t least = kind == PCOA_GRM_SUBSET_PANEL ? 32 : 1;
  if (!keep || n_keep < least)
    return fail(src, PCOA_ERR_INVALID_ARG, "pcoa_create_grm_subset: keep is NULL or n_keep = " + std::to_string(n_keep) + " is below " +
                                               std::to_string(least) + (kind == PCOA_GRM_SUBSET_PANEL
                                                                            ? " (a panel's computePca is the Lanczos iteration, which starts at 32 samples)"
                                                                            : " (a study store holds one sample or more)"));
  for (int32_t a = 0; a < n_keep; ++a) {
    if (keep[a] < 0 || keep[a] >= src->n)
      return fail(src, PCOA_ERR_INVALID_ARG, "pcoa_create_grm_subset: keep[" + std::to_string(a) + "] = " + std::to_string(keep[a]) +
                                                 " is outside [0, " + std::to_string(src->n) + ")");
    if (a > 0 && keep[a] <= keep[a - 1])
      return fail(src, PCOA_ERR_INVALID_ARG, "pcoa_create_grm_subset: keep must be strictly increasing (keep[" + std::to_string(a) +
                                                 "] = " + std::to_string(keep[a]) + " follows " + std::to_string(keep[a - 1]) + ")");
  }
  CHECK_CTX(src);
  int rc = check_device_flags(src);   // synchronises src
  if (rc != PCOA_OK) return rc;

  pcoa_ctx* sub = nullptr;
  rc = kind == PCOA_GRM_SUBSET_PANEL ? create_grm_engine(&sub, n_keep, src->device, src->flags)
                                     : create_grm_study_engine(&sub, n_keep, src->device, src->flags);
  if (rc != PCOA_OK) return fail(src, rc, std::string("pcoa_create_grm_subset: the new engine: ") + pcoa_last_error(nullptr));
  sub->grm_min_maf = src->grm_min_maf;
  sub->grm_max_missing = src->grm_max_missing;   // the variant filters are inherited like min_maf; the counts, p-values and
  sub->grm_hwe_min_p = src->grm_hwe_min_p;       // used_v are re-derived from the subset's own columns
  // from here on a failure is reported on src and takes the half-built engine with it
  int32_t* keep_dev = nullptr;
  auto bail = [&](int code, std::string msg) {   // by value: the message usually lives in the engine destroyed below
    (void)hipStreamSynchronize(src->stream);
    if (keep_dev) dev_free(keep_dev);
    pcoa_destroy(sub);
    (void)hipSetDevice(src->device);
    return fail(src, code, "pcoa_create_grm_subset: " + msg + "; src is as it was");
  };
  auto hip_bail = [&](hipError_t e, const char* what) {
    const int code = hip_fail(sub, e, what);
    return bail(code, sub->last_error);
  };
  const int64_t rows = src->op_variants, spitch = store_pitch_words(src), dpitch = store_pitch_words(sub);
  if ((rc = store_grow(sub, rows)) != PCOA_OK) return bail(rc, "the result's store: " + sub->last_error);
  hipError_t e;
  if ((e = dev_alloc((void**)&keep_dev, sizeof(int32_t) * (size_t)n_keep, src->device)) != hipSuccess)
    return hip_bail(e, "allocation of the kept indices");
  if ((e = hipMemcpyAsync(keep_dev, keep, sizeof(int32_t) * (size_t)n_keep, hipMemcpyHostToDevice, src->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(keep)");
  {
    ScopedTimer t(src, T_GRM_SUBSET);
    for (const auto& s : src->op_segs) {
      rc = store_append(sub, s.rows, [&](int64_t done, int64_t cur, uint32_t* dst) {
        return launch_grm_subset(s.p + done * spitch, cur, src->n, keep_dev, n_keep, dst, src->num_cu, src->stream);
      });
      if (rc != PCOA_OK) break;
    }
  }
  if (rc != PCOA_OK) return bail(rc, "grm_subset_kernel: " + sub->last_error);
  if ((e = hipStreamSynchronize(src->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  dev_free(keep_dev);
  keep_dev = nullptr;
  src->grm_subset_calls += 1;
  src->grm_subset_bytes += rows * (spitch + dpitch) * 4;
  (void)hipSetDevice(src->device);
  *out = sub;
  return PCOA_OK;
}

int pcoa_grm_rows(pcoa_ctx* c, int64_t first_variant, int64_t n_variants, uint8_t* out) {
  CHECK_CTX(c);
  if (!c->is_grm)
    return fail(c, PCOA_ERR_STATE, std::string("pcoa_grm_rows: not a GRM ctx (pcoa_create_grm, pcoa_create_grm_study) but ") + kind_of(c));
  if (first_variant < 0 || n_variants < 0 || first_variant > c->op_variants || n_variants > c->op_variants - first_variant)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_rows: rows [" + std::to_string(first_variant) + ", " +
                                             std::to_string(first_variant + n_variants) + ") are not inside the store's " +
                                             std::to_string(c->op_variants));
  if (!out) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_rows: out is NULL");
  if (n_variants == 0) return PCOA_OK;
  const int rc = check_device_flags(c);
  if (rc != PCOA_OK) return rc;
  const int64_t pitch = store_pitch_words(c), nb = ((int64_t)c->n + 3) / 4, a = first_variant, b = first_variant + n_variants;
  int64_t row0 = 0;
  for (const auto& s : c->op_segs) {
    const int64_t lo = std::max(a, row0), hi = std::min(b, row0 + s.rows);
    if (lo < hi)
      HIP_TRY(c, hipMemcpy2DAsync(out + (lo - a) * nb, (size_t)nb, s.p + (lo - row0) * pitch, (size_t)pitch * 4, (size_t)nb, (size_t)(hi - lo),
                                  hipMemcpyDeviceToHost, c->stream));
    row0 += s.rows;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->n % 4 != 0) {   // the unused slots of a row's last byte are 00 in a .bed row (01 in the store)
    const uint8_t live = (uint8_t)((1u << (2 * (c->n % 4))) - 1u);
    for (int64_t r = 0; r < n_variants; ++r) out[r * nb + nb - 1] &= live;
  }
  return PCOA_OK;
}

int pcoa_get_grm_subset_stats(pcoa_ctx* c, pcoa_grm_subset_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(double)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_grm_subset_stats full;
  std::memset(&full, 0, sizeof(full));
  full.grm_subset_seconds = c->tsec[T_GRM_SUBSET];
  full.grm_subset_calls = c->grm_subset_calls;
  full.grm_subset_bytes = c->grm_subset_bytes;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
