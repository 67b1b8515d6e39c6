// capi_grm_qc.hip -- variant and sample quality control on a GRM ctx's resident store (the rule is stated at the
// block of pcoa.h, the kernels are grm_qc.hip's): the two variant filters beside min_maf (pcoa_grm_set_variant_filters: the
// missing share of plink --geno and the Hardy-Weinberg exact test of plink --hwe, both conjuncts of used_v in
// grm_weights_kernel, so every consumer of the weights sees them and no row moves), the p-values themselves (pcoa_grm_hwe),
// the per-sample genotype counts over all or over the used rows (pcoa_grm_sample_counts) and what the three did
// (pcoa_get_grm_qc_stats).  The p-values live beside the counts and are dropped with them (capi_grm.hip's grm_counts).
#include <cmath>
#include <cstring>
#include <string>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace {

const char* kind_of(const pcoa_ctx* c) {
  if (c->is_grm_study) return "a GRM study ctx (pcoa_create_grm_study)";
  if (c->is_strip) return "a strip owner (pcoa_create_strip)";
  if (c->is_operator) return "an operator ctx (pcoa_create_operator)";
  return "a full engine (pcoa_create)";
}

// PCOA_OK, or the PCOA_ERR_STATE of a ctx that has no GRM store with weights of its own
int check_panel(pcoa_ctx* c, const char* call) {
  if (!c->is_grm || c->is_grm_study)
    return fail(c, PCOA_ERR_STATE, std::string(call) + ": not a GRM ctx with weights of its own (pcoa_create_grm) but " + kind_of(c) +
                                       ": used_v, and so the variant filters, belong to a panel's ctx");
  return PCOA_OK;
}

int check_grm(pcoa_ctx* c, const char* call) {
  if (!c->is_grm)
    return fail(c, PCOA_ERR_STATE, std::string(call) + ": not a GRM ctx (pcoa_create_grm, pcoa_create_grm_study) but " + kind_of(c) +
                                       ": there is no genotype store");
  return PCOA_OK;
}

}  // namespace

namespace pcoa {

int grm_resident_hwe(pcoa_ctx* c) {
  int rc = grm_resident_counts(c);
  if (rc != PCOA_OK) return rc;
  if (c->grm_hwe_set) return PCOA_OK;
  if ((rc = ensure(c, &c->grm_hwe, &c->grm_hwe_cap, std::max<int64_t>(c->op_variants, 1))) != PCOA_OK) return rc;
  {
    ScopedTimer t(c, T_GRM_QC_HWE);
    HIP_TRY(c, launch_grm_hwe(c->grm_cnt, c->op_variants, c->grm_hwe, c->stream));
  }
  c->grm_hwe_calls += 1;
  c->grm_hwe_set = true;
  return PCOA_OK;
}

void grm_qc_destroy(pcoa_ctx* c) {
  if (c->grm_hwe) dev_free(c->grm_hwe);
  if (c->grm_qc_part) dev_free(c->grm_qc_part);
  if (c->grm_qc_out) dev_free(c->grm_qc_out);
  c->grm_hwe = nullptr;
  c->grm_qc_part = nullptr;
  c->grm_qc_out = nullptr;
  c->grm_hwe_set = false;
}

}  // namespace pcoa

extern "C" {

int pcoa_grm_set_variant_filters(pcoa_ctx* c, double max_missing, double hwe_min_p) {
  CHECK_CTX(c);
  const int rc = check_panel(c, "pcoa_grm_set_variant_filters");
  if (rc != PCOA_OK) return rc;
  if (!(max_missing >= 0.0 && max_missing <= 1.0))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_set_variant_filters: max_missing = " + std::to_string(max_missing) + " is outside [0, 1]");
  if (!(hwe_min_p >= 0.0 && hwe_min_p < 1.0))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_set_variant_filters: hwe_min_p = " + std::to_string(hwe_min_p) + " is outside [0, 1)");
  if (hwe_min_p > 0.0 && (int64_t)c->n >= ((int64_t)1 << 26))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_set_variant_filters: hwe_min_p > 0 with N = " + std::to_string(c->n) +
                                             " samples: the exact test's tie rule needs N < 2^26");
  if (max_missing != c->grm_max_missing || hwe_min_p != c->grm_hwe_min_p) {
    c->grm_weights_set = false;
    grm_ld_drop(c);   // the mask was judged under the old filters
  }
  c->grm_max_missing = max_missing;
  c->grm_hwe_min_p = hwe_min_p;
  return PCOA_OK;
}

int pcoa_grm_get_variant_filters(const pcoa_ctx* c, double* max_missing_out, double* hwe_min_p_out) {
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_grm_get_variant_filters: ctx is NULL");
  const int rc = check_panel(const_cast<pcoa_ctx*>(c), "pcoa_grm_get_variant_filters");
  if (rc != PCOA_OK) return rc;
  if (max_missing_out) *max_missing_out = c->grm_max_missing;
  if (hwe_min_p_out) *hwe_min_p_out = c->grm_hwe_min_p;
  return PCOA_OK;
}

int pcoa_grm_hwe(pcoa_ctx* c, int64_t first_variant, int64_t n_variants, double* out) {
  CHECK_CTX(c);
  int rc = check_grm(c, "pcoa_grm_hwe");
  if (rc != PCOA_OK) return rc;
  if (first_variant < 0 || n_variants < 0 || first_variant > c->op_variants || n_variants > c->op_variants - first_variant)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_hwe: rows [" + std::to_string(first_variant) + ", " +
                                             std::to_string(first_variant + n_variants) + ") are not inside the store's " +
                                             std::to_string(c->op_variants));
  if (n_variants > 0 && !out) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_hwe: out is NULL");
  if (n_variants == 0) return PCOA_OK;
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  if ((rc = grm_resident_hwe(c)) != PCOA_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(out, c->grm_hwe + first_variant, sizeof(double) * (size_t)n_variants, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

int pcoa_grm_sample_counts(pcoa_ctx* c, int32_t rows, int64_t* out) {
  CHECK_CTX(c);
  int rc = check_grm(c, "pcoa_grm_sample_counts");
  if (rc != PCOA_OK) return rc;
  if (rows != PCOA_GRM_ROWS_ALL && rows != PCOA_GRM_ROWS_USED)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_sample_counts: rows = " + std::to_string(rows) +
                                             " is neither PCOA_GRM_ROWS_ALL (0) nor PCOA_GRM_ROWS_USED (1)");
  if (rows == PCOA_GRM_ROWS_USED && c->is_grm_study)
    return fail(c, PCOA_ERR_STATE, "pcoa_grm_sample_counts: PCOA_GRM_ROWS_USED on a GRM study ctx (pcoa_create_grm_study), which has no "
                                   "used_v of its own; PCOA_GRM_ROWS_ALL counts every row of its store");
  if (!out) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_sample_counts: out is NULL");
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  const int32_t* used = nullptr;
  int64_t counted = c->op_variants;
  if (rows == PCOA_GRM_ROWS_USED) {
    if ((rc = grm_resident_weights(c)) != PCOA_OK) return rc;
    used = grm_used_rows(c);
    counted = c->grm_used;
  }
  const int64_t ranges = grm_store_ranges(c), ystride = (int64_t)grm_pitch_words(c->n) * 16;
  if ((rc = ensure(c, &c->grm_qc_part, &c->grm_qc_part_cap, std::max<int64_t>(ranges, 1) * 3 * ystride)) != PCOA_OK) return rc;
  if ((rc = ensure(c, &c->grm_qc_out, &c->grm_qc_out_cap, (int64_t)c->n * 3 + 3)) != PCOA_OK) return rc;
  {
    ScopedTimer t(c, T_GRM_QC_SAMPLES);
    int64_t row0 = 0, q0 = 0;
    for (const auto& s : c->op_segs) {
      HIP_TRY(c, launch_grm_sample_counts(s.p, (int32_t)s.rows, c->n, used ? used + row0 : nullptr, c->grm_qc_part + q0 * 3 * ystride,
                                          c->stream));
      row0 += s.rows;
      q0 += (s.rows + kGrmRangeRows - 1) / kGrmRangeRows;
    }
    HIP_TRY(c, launch_grm_sample_counts_finish(c->grm_qc_part, (int32_t)ranges, c->n, counted, c->grm_qc_out, c->stream));
  }
  c->grm_sample_counts_calls += 1;
  HIP_TRY(c, hipMemcpyAsync(out, c->grm_qc_out, sizeof(int64_t) * 3 * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

int pcoa_get_grm_qc_stats(pcoa_ctx* c, pcoa_grm_qc_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(double)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc = fp4_sync_point(c);
  if (rc != PCOA_OK) return rc;
  pcoa_grm_qc_stats full;
  std::memset(&full, 0, sizeof(full));
  if (c->is_grm && !c->is_grm_study && c->op_variants > 0) {   // the fail counts under the current settings
    const bool hwe = c->grm_hwe_min_p > 0.0;
    if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
    if ((rc = hwe ? grm_resident_hwe(c) : grm_resident_counts(c)) != PCOA_OK) return rc;
    if ((rc = ensure(c, &c->grm_qc_out, &c->grm_qc_out_cap, (int64_t)c->n * 3 + 3)) != PCOA_OK) return rc;
    unsigned long long* fails = reinterpret_cast<unsigned long long*>(c->grm_qc_out + (int64_t)c->n * 3);
    HIP_TRY(c, hipMemsetAsync(fails, 0, sizeof(unsigned long long) * 3, c->stream));
    HIP_TRY(c, launch_grm_qc_fails(c->grm_cnt, c->op_variants, c->n, c->grm_min_maf, c->grm_max_missing, c->grm_hwe_min_p,
                                   hwe ? c->grm_hwe : nullptr, fails, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->hw->qc, fails, sizeof(int64_t) * 3, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    full.grm_qc_fail_maf = c->hw->qc[0];
    full.grm_qc_fail_missing = c->hw->qc[1];
    full.grm_qc_fail_hwe = c->hw->qc[2];
  }
  drain_events(c, true);
  full.grm_qc_hwe_seconds = c->tsec[T_GRM_QC_HWE];
  full.grm_qc_hwe_calls = c->grm_hwe_calls;
  full.grm_qc_sample_counts_seconds = c->tsec[T_GRM_QC_SAMPLES];
  full.grm_qc_sample_counts_calls = c->grm_sample_counts_calls;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
