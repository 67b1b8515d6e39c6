// capi_grm_pcrelate.hip -- PC-Relate kinship on the resident 2-bit store of a GRM ctx (the rule is stated at
// pcoa_grm_pcrelate_block in pcoa.h, the kernels are grm_pcrelate.hip's).  pcoa_pcrelate_hat is pure host arithmetic: the
// pseudo-inverse of the covariates, so that both hosts and Python hold the same bits.  pcoa_grm_pcrelate_fit regresses the dosages
// on the covariates -- pass 1 of grm_multi.hip applied to the rows of hat, two at a time -- and leaves beta and the basis resident;
// the block call runs one launch per segment of the store and one division per entry; the pairs call walks the upper triangle in
// bands with grm_pairs.hip's count / scan / write on the phi band and the n band.  Nothing here writes the store.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace {

const char* kind_of(const pcoa_ctx* c) {
  if (c->is_strip) return "a strip owner (pcoa_create_strip)";
  if (c->is_operator) return "an operator ctx (pcoa_create_operator)";
  return "a full engine (pcoa_create)";
}

constexpr int32_t kPcrDefaultBandRows = 1024;

// what every call asks of the ctx's kind
int check_kind(pcoa_ctx* c, const std::string& fn) {
  if (!c->is_grm)
    return fail(c, PCOA_ERR_STATE, fn + ": not a GRM ctx (pcoa_create_grm) but " + kind_of(c) + ": there is no genotype store to fit");
  if (c->is_grm_study)
    return fail(c, PCOA_ERR_STATE, fn + ": a GRM study ctx (pcoa_create_grm_study) holds the genotypes of study samples and "
                                        "no weights of its own; pass it to pcoa_grm_project beside the panel's ctx");
  return PCOA_OK;
}

int check_fit(pcoa_ctx* c, const std::string& fn) {
  if (c->grm_pcr_set) return PCOA_OK;
  const char* why = c->grm_pcr_dropped_by == 1   ? ": pcoa_accumulate_plink_bed dropped it (the store has rows the fit never saw)"
                    : c->grm_pcr_dropped_by == 2 ? ": pcoa_reset dropped it"
                    : c->grm_pcr_dropped_by == 3 ? ": a later pcoa_grm_pcrelate_fit that failed overwrote it"
                                                 : "";
  return fail(c, PCOA_ERR_STATE, fn + ": no fit on this ctx (pcoa_grm_pcrelate_fit)" + why);
}

int check_threshold(pcoa_ctx* c, const std::string& fn, double t) {
  if (!std::isfinite(t) || !(t >= 0.0 && t < 0.5))
    return fail(c, PCOA_ERR_INVALID_ARG, fn + ": maf_threshold = " + std::to_string(t) + " is not a finite number in [0, 0.5)");
  return PCOA_OK;
}

// the weights resident, M' in (0, 2^31)
int check_used(pcoa_ctx* c, const std::string& fn, GrmParams* g, int64_t* used) {
  const int rc = grm_resident_params(c, g, used);
  if (rc != PCOA_OK) return rc;
  if (*used == 0)
    return fail(c, PCOA_ERR_STATE, fn + ": none of the " + std::to_string(c->op_variants) +
                                       " variants in the store is used (polymorphic, called, at or above min_maf): M' = 0");
  if (*used >= ((int64_t)1 << 31))
    return fail(c, PCOA_ERR_STATE, fn + ": M' = " + std::to_string(*used) + " used variants do not fit the int32 pair counts");
  return PCOA_OK;
}

int check_window(pcoa_ctx* c, const std::string& fn, int64_t first, int64_t nv, const void* out) {
  const int64_t v = c->op_variants;
  if (first < 0 || nv < 0 || first > v || nv > v - first)
    return fail(c, PCOA_ERR_INVALID_ARG, fn + ": rows [" + std::to_string(first) + ", " + std::to_string(first + nv) +
                                             ") are not inside the store's " + std::to_string(v));
  if (!out) return fail(c, PCOA_ERR_INVALID_ARG, fn + ": out is NULL");
  return PCOA_OK;
}

}  // namespace

extern "C" {

int pcoa_pcrelate_hat(int32_t n_cov, int32_t n, const double* basis, double* hat_out) {
#pragma clang fp contract(off)
  if (n_cov < 1 || n_cov > kGrmPcrelateMaxCov)
    return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_pcrelate_hat: n_cov = " + std::to_string(n_cov) + " is outside [1, " +
                                                   std::to_string(kGrmPcrelateMaxCov) + "]");
  if (n < n_cov)
    return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_pcrelate_hat: n = " + std::to_string(n) + " samples cannot determine n_cov = " +
                                                   std::to_string(n_cov) + " covariates");
  if (!basis || !hat_out) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_pcrelate_hat: basis or hat_out is NULL");
  for (int64_t e = 0; e < (int64_t)n_cov * n; ++e)
    if (!std::isfinite(basis[e]))
      return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_pcrelate_hat: basis[" + std::to_string(e / n) + "][" + std::to_string(e % n) +
                                                     "] is not a finite number");
  // G packed, h[c][j] at c (c + 1) / 2 + j, j <= c
  double h[kGrmPcrelateMaxCov * (kGrmPcrelateMaxCov + 1) / 2];
  auto at = [&](int c, int j) -> double& { return h[c * (c + 1) / 2 + j]; };
  for (int c = 0; c < n_cov; ++c)
    for (int j = 0; j <= c; ++j) {
      const double *bc = basis + (int64_t)c * n, *bj = basis + (int64_t)j * n;
      double s = 0.0;
      for (int32_t i = 0; i < n; ++i) {
        const double p = bc[i] * bj[i];
        s = s + p;
      }
      at(c, j) = s;
    }
  // the square-root-free LDL^T of pcoa_grm_project_lsq's header, in its sequence
  for (int c = 0; c < n_cov; ++c) {
    const double hcc = at(c, c);
    for (int j = 0; j < c; ++j) {
      double s = at(c, j);
      for (int k = 0; k < j; ++k) {
        const double p = at(c, k) * at(j, k);
        s = s - p;
      }
      at(c, j) = s;
    }
    double s = hcc;
    for (int k = 0; k < c; ++k) {
      const double w = at(c, k);
      const double l = w / at(k, k);
      const double p = w * l;
      s = s - p;
      at(c, k) = l;
    }
    if (!(hcc > 0.0) || !std::isfinite(s) || s <= 0x1p-40 * hcc)
      return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_pcrelate_hat: covariate " + std::to_string(c) +
                                                     " is collinear with the covariates before it (pivot " + std::to_string(s) +
                                                     " <= 2^-40 * G[c][c] = " + std::to_string(0x1p-40 * hcc) + ")");
    at(c, c) = s;
  }
  // forward / diagonal / backward per sample column
  for (int32_t i = 0; i < n; ++i) {
    double y[kGrmPcrelateMaxCov], x[kGrmPcrelateMaxCov];
    for (int c = 0; c < n_cov; ++c) {
      double s = basis[(int64_t)c * n + i];
      for (int k = 0; k < c; ++k) {
        const double p = at(c, k) * y[k];
        s = s - p;
      }
      y[c] = s;
    }
    for (int c = 0; c < n_cov; ++c) y[c] = y[c] / at(c, c);
    for (int c = n_cov - 1; c >= 0; --c) {
      double s = y[c];
      for (int k = c + 1; k < n_cov; ++k) {
        const double p = at(k, c) * x[k];
        s = s - p;
      }
      x[c] = s;
    }
    for (int c = 0; c < n_cov; ++c) hat_out[(int64_t)c * n + i] = x[c];
  }
  return PCOA_OK;
}

int pcoa_grm_pcrelate_fit(pcoa_ctx* c, int32_t n_cov, const double* basis, const double* hat) {
#pragma clang fp contract(off)
  const std::string fn = "pcoa_grm_pcrelate_fit";
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, fn + ": ctx is NULL");
  if (!basis || !hat) return fail(c, PCOA_ERR_INVALID_ARG, fn + ": basis or hat is NULL");
  if (n_cov < 1 || n_cov > kGrmPcrelateMaxCov)
    return fail(c, PCOA_ERR_INVALID_ARG, fn + ": n_cov = " + std::to_string(n_cov) + " is outside [1, " +
                                             std::to_string(kGrmPcrelateMaxCov) + "]");
  int rc = check_kind(c, fn);
  if (rc != PCOA_OK) return rc;
  const int64_t n = c->n, v = c->op_variants;
  for (int64_t e = 0; e < (int64_t)n_cov * n; ++e) {
    const bool bad_basis = !std::isfinite(basis[e]);
    if (bad_basis || !std::isfinite(hat[e]))
      return fail(c, PCOA_ERR_INVALID_ARG, fn + ": " + (bad_basis ? "basis[" : "hat[") + std::to_string(e / n) + "][" +
                                               std::to_string(e % n) + "] is not a finite number");
  }
  if (v == 0) return fail(c, PCOA_ERR_STATE, fn + ": the store is empty: there is nothing to fit");
  CHECK_CTX(c);
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  GrmParams g;
  if ((rc = grm_resident_params(c, &g, nullptr)) != PCOA_OK) return rc;
  // S_c = sum_i hat[c][i], i ascending
  double sums[kGrmPcrelateMaxCov];
  for (int32_t k = 0; k < n_cov; ++k) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s = s + hat[(int64_t)k * n + i];
    sums[k] = s;
  }
  // the call's own layout of the ctx's multi-vector workspace, in doubles: hat [n_cov][N] | S [n_cov] | tpart [2][groups][V]
  struct { double *u, *lam, *tpart; } w;
  if ((rc = ensure(c, &c->grm_mw, &c->grm_mw_cap, (int64_t)n_cov * n + n_cov + 2 * (int64_t)grm_groups(c->n) * v)) != PCOA_OK) return rc;
  w.u = c->grm_mw;
  w.lam = w.u + (int64_t)n_cov * n;
  w.tpart = w.lam + n_cov;
  // an earlier fit stays as it is unless its buffer has to grow; from the first copy on it is being overwritten, and a failure
  // behind that point leaves the ctx without a fit and says so
  if ((int64_t)n_cov * (v + n) > c->grm_pcr_cap) grm_pcr_drop(c, 3);
  if ((rc = ensure(c, &c->grm_pcr, &c->grm_pcr_cap, (int64_t)n_cov * (v + n))) != PCOA_OK) return rc;
  grm_pcr_drop(c, 3);
  double* const beta = c->grm_pcr;
  double* const basis_dev = beta + (int64_t)n_cov * v;
  const int64_t groups = grm_groups(c->n);
  HIP_TRY(c, hipMemcpyAsync(w.u, hat, sizeof(double) * (size_t)n_cov * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(w.lam, sums, sizeof(double) * (size_t)n_cov, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(basis_dev, basis, sizeof(double) * (size_t)n_cov * (size_t)n, hipMemcpyHostToDevice, c->stream));
  {
    ScopedTimer timer(c, T_GRM_PCR_FIT);
    for (int32_t c0 = 0; c0 < n_cov;) {
      const int32_t k = grm_multi_chunk(n_cov - c0);
      int64_t row0 = 0;
      for (const auto& sg : c->op_segs) {
        HIP_TRY(c, launch_grm_ax_multi(sg.p, (int32_t)sg.rows, c->n, g.mu + row0, w.u + (int64_t)c0 * n, n, k, w.tpart + row0, v,
                                       groups * v, c->stream));
        row0 += sg.rows;
      }
      HIP_TRY(c, launch_grm_pcrelate_beta(w.tpart, v, c->n, groups * v, v, g.mu, w.lam, c0, k, n_cov, beta, c->stream));
      c0 += k;
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // sums and the caller's matrices are consumed
  c->grm_pcr_set = true;
  c->grm_pcr_cov = n_cov;
  c->grm_pcr_dropped_by = 0;
  c->grm_pcr_fits += 1;
  return PCOA_OK;
}

int pcoa_grm_pcrelate_beta(pcoa_ctx* c, int64_t first_variant, int64_t n_variants, double* out) {
  const std::string fn = "pcoa_grm_pcrelate_beta";
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, fn + ": ctx is NULL");
  int rc = check_kind(c, fn);
  if (rc != PCOA_OK) return rc;
  if ((rc = check_window(c, fn, first_variant, n_variants, out)) != PCOA_OK) return rc;
  if ((rc = check_fit(c, fn)) != PCOA_OK) return rc;
  if (n_variants == 0) return PCOA_OK;
  CHECK_CTX(c);
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  const int64_t k = c->grm_pcr_cov;
  HIP_TRY(c, hipMemcpyAsync(out, c->grm_pcr + first_variant * k, sizeof(double) * (size_t)(n_variants * k), hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

int pcoa_grm_pcrelate_isaf(pcoa_ctx* c, int64_t first_variant, int64_t n_variants, double* out) {
  const std::string fn = "pcoa_grm_pcrelate_isaf";
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, fn + ": ctx is NULL");
  int rc = check_kind(c, fn);
  if (rc != PCOA_OK) return rc;
  if ((rc = check_window(c, fn, first_variant, n_variants, out)) != PCOA_OK) return rc;
  if ((rc = check_fit(c, fn)) != PCOA_OK) return rc;
  if (n_variants == 0) return PCOA_OK;
  CHECK_CTX(c);
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  const int64_t k = c->grm_pcr_cov, n = c->n, total = n_variants * n;
  if ((rc = ensure(c, &c->grm_blk, &c->grm_blk_cap, total)) != PCOA_OK) return rc;
  HIP_TRY(c, launch_grm_pcrelate_isaf(c->grm_pcr, (int32_t)k, c->grm_pcr + k * c->op_variants, c->n, first_variant, n_variants,
                                      c->grm_blk, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out, c->grm_blk, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

int pcoa_grm_pcrelate_block(pcoa_ctx* c, int32_t row0, int32_t rows, int32_t col0, int32_t cols, double maf_threshold, double* out_phi,
                            int32_t* out_pairs, int is_device_ptr) {
  const std::string fn = "pcoa_grm_pcrelate_block";
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, fn + ": ctx is NULL");
  const std::string rect = "rows [" + std::to_string(row0) + ", " + std::to_string((int64_t)row0 + rows) + ") x columns [" +
                           std::to_string(col0) + ", " + std::to_string((int64_t)col0 + cols) + ")";
  if (rows < 1 || cols < 1) return fail(c, PCOA_ERR_INVALID_ARG, fn + ": " + rect + ": rows and cols must be at least 1");
  if (row0 < 0 || col0 < 0 || rows > c->n - row0 || cols > c->n - col0)
    return fail(c, PCOA_ERR_INVALID_ARG, fn + ": " + rect + " is not inside [0, " + std::to_string(c->n) + ")^2");
  if (!out_phi && !out_pairs) return fail(c, PCOA_ERR_INVALID_ARG, fn + ": out_phi and out_pairs are both NULL");
  int rc = check_threshold(c, fn, maf_threshold);
  if (rc != PCOA_OK) return rc;
  if ((rc = check_kind(c, fn)) != PCOA_OK) return rc;
  if ((rc = check_fit(c, fn)) != PCOA_OK) return rc;
  CHECK_CTX(c);
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  GrmParams g;
  int64_t used = 0;
  if ((rc = check_used(c, fn, &g, &used)) != PCOA_OK) return rc;

  // the accumulators: num in the caller's device memory or the ctx's block buffer, den always in the buffer, n where it is asked
  // for: [total] num | [total] den | [total] int32
  const int64_t total = (int64_t)rows * cols, v = c->op_variants;
  const bool want_n = out_pairs != nullptr;
  const bool own_num = !(is_device_ptr && out_phi), own_n = want_n && !is_device_ptr;
  if ((rc = ensure(c, &c->grm_blk, &c->grm_blk_cap, (own_num ? total : 0) + total + (own_n ? (total + 1) / 2 : 0))) != PCOA_OK) return rc;
  double* const num_dev = own_num ? c->grm_blk : out_phi;
  double* const den_dev = c->grm_blk + (own_num ? total : 0);
  int32_t* const n_dev = !want_n ? nullptr : own_n ? reinterpret_cast<int32_t*>(den_dev + total) : out_pairs;
  const int32_t k = c->grm_pcr_cov;
  const double* const beta = c->grm_pcr;
  const double* const basis = beta + (int64_t)k * v;
  {
    ScopedTimer t(c, T_GRM_PCR_DENSE);
    int64_t seg_row0 = 0;
    int first = 1;
    for (const auto& s : c->op_segs) {
      if (s.rows <= 0) continue;
      HIP_TRY(c, launch_grm_pcrelate(s.p, (int32_t)s.rows, c->n, g.used + seg_row0, beta + seg_row0 * k, k, basis, maf_threshold, row0,
                                     rows, col0, cols, first, num_dev, den_dev, n_dev, c->stream));
      seg_row0 += s.rows;
      first = 0;
    }
    if (out_phi) HIP_TRY(c, launch_grm_pcrelate_finish(num_dev, den_dev, total, c->stream));
  }
  if (out_phi && own_num) HIP_TRY(c, hipMemcpyAsync(out_phi, num_dev, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
  if (own_n) HIP_TRY(c, hipMemcpyAsync(out_pairs, n_dev, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->grm_pcr_block_calls += 1;
  c->grm_pcr_flops += 2.0 * (double)rows * (double)cols * (double)v * (want_n ? 3.0 : 2.0);
  return PCOA_OK;
}

int pcoa_grm_pcrelate_pairs(pcoa_ctx* c, double cutoff, double maf_threshold, int32_t band_rows, pcoa_grm_pair* out_pairs,
                            int64_t capacity, int64_t* n_found_out, double* out_diag) {
  const std::string fn = "pcoa_grm_pcrelate_pairs";
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, fn + ": ctx is NULL");
  if (!n_found_out) return fail(c, PCOA_ERR_INVALID_ARG, fn + ": n_found_out is NULL");
  if (!std::isfinite(cutoff)) return fail(c, PCOA_ERR_INVALID_ARG, fn + ": cutoff = " + std::to_string(cutoff) + " is not a finite number");
  int rc = check_threshold(c, fn, maf_threshold);
  if (rc != PCOA_OK) return rc;
  if (band_rows < 0 || band_rows % 64 != 0)
    return fail(c, PCOA_ERR_INVALID_ARG, fn + ": band_rows = " + std::to_string(band_rows) +
                                             " is neither 0 (1,024 rows) nor a positive multiple of 64");
  if (capacity < 0) return fail(c, PCOA_ERR_INVALID_ARG, fn + ": capacity = " + std::to_string(capacity) + " is negative");
  if (capacity > 0 && !out_pairs)
    return fail(c, PCOA_ERR_INVALID_ARG, fn + ": out_pairs is NULL with capacity = " + std::to_string(capacity) +
                                             " (capacity 0 is the count-only call)");
  if ((rc = check_kind(c, fn)) != PCOA_OK) return rc;
  if ((rc = check_fit(c, fn)) != PCOA_OK) return rc;
  CHECK_CTX(c);
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  GrmParams g;
  int64_t used = 0;
  if ((rc = check_used(c, fn, &g, &used)) != PCOA_OK) return rc;

  const int32_t n = c->n;
  const int64_t v = c->op_variants;
  const int64_t npad = ((int64_t)n + 63) / 64 * 64;   // a band's columns end here: its pitch npad - c0 is a multiple of 64 doubles
  const int32_t band = (int32_t)std::min<int64_t>(band_rows ? band_rows : kPcrDefaultBandRows, npad);
  const int64_t most = (int64_t)n * (int64_t)(n - 1) / 2;
  const int64_t cap_dev = std::min(capacity, most);
  const size_t ntiles_max = (size_t)grm_pairs_tiles(n);

  // the band, in the buffer pcoa_grm_block grows: [band][npad] num (then phi) | [band][npad] den | [band][npad] int32 n
  const int64_t band_elems = (int64_t)band * npad;
  if ((rc = ensure(c, &c->grm_blk, &c->grm_blk_cap, 2 * band_elems + (band_elems + 1) / 2)) != PCOA_OK) return rc;
  double* const num_dev = c->grm_blk;
  double* const den_dev = num_dev + band_elems;
  int32_t* const n_dev = reinterpret_cast<int32_t*>(den_dev + band_elems);
  const int32_t k = c->grm_pcr_cov;
  const double* const beta = c->grm_pcr;
  const double* const basis = beta + (int64_t)k * v;
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
      ScopedTimer t(c, T_GRM_PCR_DENSE);
      int64_t seg_row0 = 0;
      int first = 1;
      for (const auto& s : c->op_segs) {
        if (s.rows <= 0) continue;
        if ((e = launch_grm_pcrelate(s.p, (int32_t)s.rows, n, g.used + seg_row0, beta + seg_row0 * k, k, basis, maf_threshold, r0, nrows,
                                     c0, pitch, first, num_dev, den_dev, n_dev, c->stream)) != hipSuccess)
          return hip_bail(e, "grm_pcrelate_kernel");
        seg_row0 += s.rows;
        first = 0;
      }
      if ((e = launch_grm_pcrelate_finish(num_dev, den_dev, (int64_t)nrows * pitch, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_pcrelate_finish_kernel");
    }
    {
      ScopedTimer t(c, T_GRM_PCR_SCREEN);
      if ((e = launch_grm_pairs_count(num_dev, pitch, r0, nrows, c0, n, cutoff, cnt, diag, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_pairs_count_kernel");
      if ((e = launch_grm_pairs_scan(cnt, nrows, grm_pairs_tiles(n - c0), rowoff, total, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_pairs scan kernels");
      if (cap_dev > 0 && (e = launch_grm_pairs_write(num_dev, n_dev, pitch, r0, nrows, c0, n, cutoff, used, cnt, rowoff, cap_dev, pairs_dev,
                                                     entries_read, c->stream)) != hipSuccess)
        return hip_bail(e, "grm_pairs_write_kernel");
    }
    bands += 1;
    count_entries += grm_pairs_count_pass_entries(r0, nrows, c0, n);
    flops += 2.0 * (double)nrows * (double)pitch * (double)v * 3.0;
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
    return fail(c, PCOA_ERR_HIP, fn + ": the scan returned " + std::to_string(n_found) + " pairs of at most " + std::to_string(most));
  }
  const int64_t written = std::min(n_found, cap_dev);
  if (written > 0) {
    if ((e = hipMemcpyAsync(out_pairs, pairs_dev, sizeof(pcoa_grm_pair) * (size_t)written, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
      return hip_bail(e, "hipMemcpyAsync(pairs)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  }
  release();
  c->grm_pcr_pairs_calls += 1;
  c->grm_pcr_bands += bands;
  c->grm_pcr_flops += flops;
  c->grm_pcr_bytes += (int64_t)sizeof(double) * count_entries + (int64_t)(sizeof(double) + sizeof(int32_t)) * reread;
  *n_found_out = n_found;
  return PCOA_OK;
}

int pcoa_get_grm_pcrelate_stats(pcoa_ctx* c, pcoa_grm_pcrelate_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_grm_pcrelate_stats full;
  std::memset(&full, 0, sizeof(full));
  full.grm_pcrelate_fits = c->grm_pcr_fits;
  full.grm_pcrelate_block_calls = c->grm_pcr_block_calls;
  full.grm_pcrelate_pairs_calls = c->grm_pcr_pairs_calls;
  full.grm_pcrelate_bands = c->grm_pcr_bands;
  full.grm_pcrelate_fit_seconds = c->tsec[T_GRM_PCR_FIT];
  full.grm_pcrelate_dense_seconds = c->tsec[T_GRM_PCR_DENSE];
  full.grm_pcrelate_screen_seconds = c->tsec[T_GRM_PCR_SCREEN];
  full.grm_pcrelate_flops = c->grm_pcr_flops;
  full.grm_pcrelate_bytes = c->grm_pcr_bytes;
  full.grm_pcrelate_n_cov = c->grm_pcr_set ? c->grm_pcr_cov : 0;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
