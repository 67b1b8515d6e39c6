// capi_grm.hip -- the standardised-genotype operator of the C ABI (pcoa_create_grm): a ctx that keeps the 2-bit
// genotype rows of a PLINK fileset and applies K = A^T diag(d) A / M' -- the genetic relationship matrix of smartpca, plink
// --pca, GCTA and flashpca over allele-frequency-standardised dosages, missing calls mean-imputed -- to a vector as two passes
// over them (grm_bits.hip).  The ctx is an operator ctx with another row format: the segmented store, reset, reserve and
// destroy are capi_operator.hip's.  Here: the .bed boundary into the store, the per-variant counts and weights (resident until
// the store or min_maf changes), the product, and computePca as the engine's Lanczos iteration over that product.
#include <algorithm>
#include <string>

#include "pcoa_ctx.h"
#include "row_feed.h"

using namespace pcoa;

namespace {

int64_t store_ranges(const pcoa_ctx* c) {
  int64_t q = 0;
  for (const auto& s : c->op_segs) q += (s.rows + kGrmRangeRows - 1) / kGrmRangeRows;
  return q;
}

// layout of grm_par, in doubles: M' (a 64-bit count) | mu [V] | d [V]; of grm_cnt, in int32: counts [V][3] | used [V]
struct GrmWeights {
  unsigned long long* mprime;
  double *mu, *d;
  int32_t *cnt, *used;
};

GrmWeights weights_of(const pcoa_ctx* c) {
  const int64_t v = std::max<int64_t>(c->op_variants, 1);
  GrmWeights w;
  w.mprime = reinterpret_cast<unsigned long long*>(c->grm_par);
  w.mu = c->grm_par + 1;
  w.d = w.mu + v;
  w.cnt = c->grm_cnt;
  w.used = w.cnt + 3 * v;
  return w;
}

// layout of op_ws, in doubles: t [V] | s [V] | tpart [groups][V] | ypart [ranges][pitch * 16].  The integer twin of the second
// pass uses ypart's memory for its int32 partials.
struct GrmWorkspace {
  double *t, *s, *tpart, *ypart;
  int64_t vstride, ranges;
};

int ensure_grm_ws(pcoa_ctx* c, GrmWorkspace* w) {
  const int64_t v = std::max<int64_t>(c->op_variants, 1), groups = grm_groups(c->n);
  const int64_t ranges = std::max<int64_t>(store_ranges(c), 1), ystride = (int64_t)grm_pitch_words(c->n) * 16;
  const int rc = ensure(c, &c->op_ws, &c->op_ws_cap, 2 * v + groups * v + ranges * ystride);
  if (rc != PCOA_OK) return rc;
  w->t = c->op_ws;
  w->s = w->t + v;
  w->tpart = w->s + v;
  w->ypart = w->tpart + groups * v;
  w->vstride = v;
  w->ranges = store_ranges(c);
  return PCOA_OK;
}

// n_v, h_v, o_v of every row of the store; resident until the store changes
int grm_counts(pcoa_ctx* c) {
  if (c->op_centering_set) return PCOA_OK;
  const int64_t v = std::max<int64_t>(c->op_variants, 1);
  int rc = ensure(c, &c->grm_cnt, &c->grm_cnt_cap, 4 * v);
  if (rc != PCOA_OK) return rc;
  if ((rc = ensure(c, &c->grm_par, &c->grm_par_cap, 1 + 2 * v)) != PCOA_OK) return rc;
  {
    ScopedTimer t(c, T_CENTER);
    int64_t row0 = 0;
    for (const auto& s : c->op_segs) {
      HIP_TRY(c, launch_grm_counts(s.p, (int32_t)s.rows, c->n, c->grm_cnt + 3 * row0, c->stream));
      row0 += s.rows;
    }
  }
  c->op_centering_set = true;
  c->grm_weights_set = false;
  c->grm_hwe_set = false;   // the p-values are dropped with the counts they were computed from
  return PCOA_OK;
}

// mu, d, used and M' from the counts, min_maf, the variant filters and (with_mask) the LD keep mask, into the resident arrays.
// The p-values are computed first where the HWE filter is on.  The host learns M' here.
int weights_pass(pcoa_ctx* c, bool with_mask) {
  const bool hwe = c->grm_hwe_min_p > 0.0;
  if (hwe) {
    const int rc = grm_resident_hwe(c);
    if (rc != PCOA_OK) return rc;
  }
  const GrmWeights w = weights_of(c);
  {
    ScopedTimer t(c, T_CENTER);
    HIP_TRY(c, hipMemsetAsync(w.mprime, 0, sizeof(unsigned long long), c->stream));
    HIP_TRY(c, launch_grm_weights(w.cnt, c->op_variants, c->grm_min_maf, with_mask ? c->grm_keep : nullptr, c->n, c->grm_max_missing,
                                  c->grm_hwe_min_p, hwe ? c->grm_hwe : nullptr, w.mu, w.d, w.used, w.mprime, c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(&c->hw->grm[0], w.mprime, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->grm_used = c->hw->grm[0];
  return PCOA_OK;
}

// the weights under the counts, min_maf and the keep mask where one is installed; resident until one of them changes
int grm_weights(pcoa_ctx* c) {
  int rc = grm_counts(c);
  if (rc != PCOA_OK) return rc;
  if (c->grm_weights_set) return PCOA_OK;
  if ((rc = weights_pass(c, c->grm_keep_set)) != PCOA_OK) return rc;
  c->grm_weights_set = true;
  return PCOA_OK;
}

// one product on the ctx stream (queued, not waited for): y = K x
hipError_t grm_product(pcoa_ctx* c, const GrmWorkspace& w, const double* x, double* y) {
  hipError_t e = hipSuccess;
  const GrmWeights g = weights_of(c);
  const int64_t ystride = (int64_t)grm_pitch_words(c->n) * 16;
  int64_t row0 = 0;
  for (const auto& s : c->op_segs) {
    if ((e = launch_grm_ax(s.p, (int32_t)s.rows, c->n, g.mu + row0, x, w.tpart + row0, w.vstride, c->stream)) != hipSuccess) return e;
    row0 += s.rows;
  }
  if ((e = launch_grm_combine_t(w.tpart, w.vstride, c->n, c->op_variants, g.mu, g.d, w.t, w.s, c->stream)) != hipSuccess) return e;
  int64_t q0 = 0;
  row0 = 0;
  for (const auto& s : c->op_segs) {
    if ((e = launch_grm_at(s.p, (int32_t)s.rows, c->n, w.t + row0, w.s + row0, w.ypart + q0 * ystride, c->stream)) != hipSuccess) return e;
    row0 += s.rows;
    q0 += (s.rows + kGrmRangeRows - 1) / kGrmRangeRows;
  }
  c->op_products += 1;
  return launch_grm_finish(w.ypart, (int32_t)w.ranges, c->n, g.mprime, y, c->stream);
}

// the samples called at one or more used variants -> c->hw->nz (queued)
int grm_called_samples(pcoa_ctx* c, const GrmWorkspace& w) {
  const GrmWeights g = weights_of(c);
  const int64_t ystride = (int64_t)grm_pitch_words(c->n) * 16;
  int32_t* ipart = reinterpret_cast<int32_t*>(w.ypart);
  ScopedTimer t(c, T_CENTER);
  int64_t row0 = 0, q0 = 0;
  for (const auto& s : c->op_segs) {
    HIP_TRY(c, launch_grm_called(s.p, (int32_t)s.rows, c->n, g.used + row0, ipart + q0 * ystride, c->stream));
    row0 += s.rows;
    q0 += (s.rows + kGrmRangeRows - 1) / kGrmRangeRows;
  }
  HIP_TRY(c, hipMemsetAsync(c->nz, 0, sizeof(int32_t), c->stream));
  HIP_TRY(c, launch_grm_called_finish(ipart, (int32_t)w.ranges, c->n, c->nz, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&c->hw->nz, c->nz, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  return PCOA_OK;
}

const char* kNotGrm = "not a GRM ctx (pcoa_create_grm)";

// a study store (pcoa_create_grm_study) has no weights of its own: the panel's are applied to it
int no_weights_on_study(pcoa_ctx* c, const char* call) {
  return fail(c, PCOA_ERR_STATE, std::string(call) + ": a GRM study ctx (pcoa_create_grm_study) holds the genotypes of study samples and "
                                     "no weights of its own; pass it to pcoa_grm_project beside the panel's ctx");
}

}  // namespace

namespace pcoa {

int64_t grm_store_ranges(const pcoa_ctx* c) { return store_ranges(c); }
int grm_resident_counts(pcoa_ctx* c) { return grm_counts(c); }
int grm_resident_weights(pcoa_ctx* c) { return grm_weights(c); }
const int32_t* grm_used_rows(const pcoa_ctx* c) { return weights_of(c).used; }

int grm_unmasked_used(pcoa_ctx* c, const int32_t** used_out) {
  int rc = grm_counts(c);
  if (rc != PCOA_OK) return rc;
  if (c->grm_keep_set || !c->grm_weights_set) {
    c->grm_weights_set = false;
    if ((rc = weights_pass(c, false)) != PCOA_OK) return rc;
    c->grm_weights_set = !c->grm_keep_set;
  }
  *used_out = weights_of(c).used;
  return PCOA_OK;
}

int grm_resident_params(pcoa_ctx* c, GrmParams* out, int64_t* used_out) {
  const int rc = grm_weights(c);
  if (rc != PCOA_OK) return rc;
  const GrmWeights w = weights_of(c);
  out->mprime = w.mprime;
  out->mu = w.mu;
  out->d = w.d;
  out->used = w.used;
  if (used_out) *used_out = c->grm_used;
  return PCOA_OK;
}

// pcoa_accumulate_plink_bed on a GRM ctx: the raw rows of a chunk are re-pitched straight into the store (the append kernel is
// the staging slot's only reader).  Every segment the call needs is allocated before its first row moves.
int grm_accumulate_bed(pcoa_ctx* c, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes, int ref_is_a1, int source) {
  int rc = store_grow(c, n_variants);
  if (rc != PCOA_OK) return rc;
  const int64_t slot_rows = std::min<int64_t>((int64_t)1 << 17, ((int64_t)256 << 20) / row_bytes);
  const int64_t rows_cap = std::max<int64_t>(1, std::min<int64_t>(n_variants, slot_rows));
  const int swap = ref_is_a1 ? 0 : 1;   // 11 is the homozygous NON-reference code of the store
  return feed_bed(c, bed_rows, n_variants, row_bytes, rows_cap, source, true,
                  [&](const uint8_t* src, int64_t, int64_t rows) {
                    return store_append(c, rows, [&](int64_t done, int64_t cur, uint32_t* dst) {
                      return launch_grm_append(src + done * row_bytes, row_bytes, cur, c->n, swap, dst, c->stream);
                    });
                  },
                  [](int64_t, int64_t) { return PCOA_OK; });
}

// computePca over the store: the weights, the called samples, then the engine's Lanczos with the product K x.  A pair comes
// back only with its true residual verified; there is no dense fallback (no matrix).
int grm_compute(pcoa_ctx* c, int32_t num_pc, double* out_components, double* out_eigenvalues, int32_t* out_nonzero_rows) {
  const double t0 = wall_now();
  if (c->is_grm_study) return no_weights_on_study(c, "pcoa_compute");
  int rc = check_device_flags(c);
  if (rc != PCOA_OK) return rc;
  if ((rc = ensure_workspace(c, num_pc)) != PCOA_OK) return rc;
  if ((rc = grm_weights(c)) != PCOA_OK) return rc;
  if (c->grm_used == 0)
    return fail(c, PCOA_ERR_STATE, "pcoa_compute on a GRM ctx: none of the " + std::to_string(c->op_variants) +
                                       " variants in the store is used (polymorphic, called, at or above min_maf): K is undefined");
  GrmWorkspace w;
  if ((rc = ensure_grm_ws(c, &w)) != PCOA_OK) return rc;
  if ((rc = grm_called_samples(c, w)) != PCOA_OK) return rc;
  std::string mv_error;
  LanczosMatvec mv = [&](const double* v, double* y) -> int {
    ScopedTimer t(c, T_OPERATOR);
    const hipError_t e = grm_product(c, w, v, y);
    if (e == hipSuccess) return 0;
    mv_error = std::string("GRM product: ") + hipGetErrorString(e);
    return 1;
  };
  c->eig_method = 0;
  c->eig_dense_form = 0;
  c->matvec_form = 3;
  rc = lanczos_over(c, num_pc, mv, out_components, out_eigenvalues, nullptr);
  if (rc != PCOA_OK && !mv_error.empty()) c->last_error = mv_error;
  if (rc != PCOA_OK) return rc;
  if (out_nonzero_rows) *out_nonzero_rows = c->hw->nz;
  c->compute_total = wall_now() - t0;
  return PCOA_OK;
}

void grm_destroy(pcoa_ctx* c) {
  if (c->grm_cnt) dev_free(c->grm_cnt);
  if (c->grm_par) dev_free(c->grm_par);
  if (c->grm_mw) dev_free(c->grm_mw);
  if (c->grm_blk) dev_free(c->grm_blk);
  if (c->grm_keep) dev_free(c->grm_keep);
  if (c->grm_pcr) dev_free(c->grm_pcr);
  c->grm_pcr = nullptr;
  c->grm_pcr_set = false;
  grm_qc_destroy(c);
  c->grm_keep = nullptr;
  c->grm_keep_set = false;
  c->grm_cnt = nullptr;
  c->grm_par = nullptr;
  c->grm_mw = nullptr;
  c->grm_blk = nullptr;
}

}  // namespace pcoa

extern "C" {

int pcoa_create_grm(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags) {
  return create_grm_engine(out, n_samples, device_ordinal, flags);
}

int pcoa_grm_info(pcoa_ctx* c, int64_t* variants_out, int64_t* used_out, int64_t* store_bytes_out) {
  CHECK_CTX(c);
  if (variants_out) *variants_out = c->is_grm ? c->op_variants : 0;
  if (used_out) *used_out = 0;
  if (store_bytes_out) *store_bytes_out = c->is_grm ? operator_store_bytes(c) : 0;
  if (!c->is_grm) return 0;
  if (used_out && !c->is_grm_study) {
    int rc = check_device_flags(c);
    if (rc != PCOA_OK) return rc;
    if ((rc = grm_weights(c)) != PCOA_OK) return rc;
    *used_out = c->grm_used;
  }
  return 1;
}

int pcoa_grm_set_min_maf(pcoa_ctx* c, double maf) {
  CHECK_CTX(c);
  if (!c->is_grm) return fail(c, PCOA_ERR_STATE, std::string("pcoa_grm_set_min_maf: ") + kNotGrm);
  if (c->is_grm_study) return no_weights_on_study(c, "pcoa_grm_set_min_maf");
  if (!(maf >= 0.0 && maf < 0.5))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_set_min_maf: maf = " + std::to_string(maf) + " is outside [0, 0.5)");
  if (maf != c->grm_min_maf) {
    c->grm_weights_set = false;
    grm_ld_drop(c);   // the mask was judged under the old min_maf
  }
  c->grm_min_maf = maf;
  return PCOA_OK;
}

int pcoa_grm_counts(pcoa_ctx* c, int64_t first_variant, int64_t n_variants, int32_t* out) {
  CHECK_CTX(c);
  if (!c->is_grm) return fail(c, PCOA_ERR_STATE, std::string("pcoa_grm_counts: ") + kNotGrm);
  if (first_variant < 0 || n_variants < 0 || first_variant > c->op_variants || n_variants > c->op_variants - first_variant)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_counts: rows [" + std::to_string(first_variant) + ", " +
                                             std::to_string(first_variant + n_variants) + ") are not inside the store's " +
                                             std::to_string(c->op_variants));
  if (n_variants > 0 && !out) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_counts: out is NULL");
  if (n_variants == 0) return PCOA_OK;
  int rc = check_device_flags(c);
  if (rc != PCOA_OK) return rc;
  if ((rc = grm_counts(c)) != PCOA_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(out, c->grm_cnt + 3 * first_variant, sizeof(int32_t) * 3 * (size_t)n_variants, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

int pcoa_grm_matvec_device(pcoa_ctx* c, const double* x_dev, double* y_dev) {
  CHECK_CTX(c);
  if (!c->is_grm) return fail(c, PCOA_ERR_STATE, std::string("pcoa_grm_matvec_device: ") + kNotGrm);
  if (c->is_grm_study) return no_weights_on_study(c, "pcoa_grm_matvec_device");
  if (!x_dev || !y_dev) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_matvec_device: x_dev or y_dev is NULL");
  int rc = check_device_flags(c);
  if (rc != PCOA_OK) return rc;
  if ((rc = grm_weights(c)) != PCOA_OK) return rc;
  GrmWorkspace w;
  if ((rc = ensure_grm_ws(c, &w)) != PCOA_OK) return rc;
  {
    ScopedTimer t(c, T_OPERATOR);
    HIP_TRY(c, grm_product(c, w, x_dev, y_dev));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // y_dev is ready for the caller's own stream
  return PCOA_OK;
}

}  // extern "C"
