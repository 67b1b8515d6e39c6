// capi_loadings.hip -- pcoa_loadings_*: the loading of every variant on the principal coordinates.  With X the
// V x N carrier bit matrix and J = I - 11^T / N, B = J S J = (X J)^T (X J): an eigenpair (u_c, lambda_c) of B is a right singular
// pair of X J, and the matching left singular vector is w_c = X (J u_c) / sqrt(lambda_c), one bit-select-sum per variant and
// component (loadings.hip).  pcoa_loadings_begin prepares the vectors ONCE on the host -- the mean as one left-to-right sum
// divided by N, u - mean, zero beyond N, the divisors sqrt(lambda_c) -- and uploads them; the calls between begin and end stream
// rows past them: caller's bitsets, raw .bed rows (decoded by plink_bed_to_bits_kernel, the rule of pcoa_accumulate_plink_bed) or
// the rows of an operator ctx's store; host rows come through the row feed (row_feed.h).  Only n, the device, the ctx stream and
// the staging slots of the ctx are used, so every kind of ctx serves; nothing here reads or writes S or the store's contents.  All device work is queued on the ctx stream,
// behind whatever accumulation is queued there.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pcoa_ctx.h"
#include "row_feed.h"

using namespace pcoa;

namespace {

constexpr int64_t kLoadingsLaunchRows = (int64_t)1 << 22;   // rows per launch (the grid stays far inside 2^31 blocks)
constexpr int64_t kLoadingsOutRows = (int64_t)1 << 16;      // rows whose results travel to a host `out` at a time
constexpr int64_t kLoadingsSlotRows = (int64_t)1 << 17;     // host rows per staging slot (and <= 256 MiB)

int not_begun(pcoa_ctx* c, const char* call) {
  return fail(c, PCOA_ERR_STATE, std::string(call) + ": no vectors are resident; call pcoa_loadings_begin first");
}

// rows on the device, readable on the ctx stream -> device `out`, every chunk of components a launch over the same rows
int launch_rows(pcoa_ctx* c, const uint32_t* bits_dev, int64_t nv, int64_t ld, double* out_dev) {
  const int64_t npad = words_of(c) * 32;
  ScopedTimer t(c, T_LOADINGS);
  for (int64_t v0 = 0; v0 < nv; v0 += kLoadingsLaunchRows) {
    const int64_t rows = std::min(kLoadingsLaunchRows, nv - v0);
    for (int32_t c0 = 0; c0 < c->ld_num_pc;) {
      const int k = loadings_chunk(c->ld_num_pc - c0);
      HIP_TRY(c, launch_loadings(bits_dev + v0 * ld, rows, ld, c->n, c->ld_u + (int64_t)c0 * npad, npad, k,
                                 c->ld_div ? c->ld_div + c0 : nullptr, out_dev + v0 * c->ld_num_pc + c0, c->ld_num_pc, c->stream));
      c->ld_bytes += rows * words_of(c) * 4;
      c0 += k;
    }
  }
  c->ld_variants += nv;
  return PCOA_OK;
}

// the same to the caller's `out`: a device `out` is written by the kernels (queued); a host `out` is filled, a chunk of rows
// at a time, through c->ld_out, and complete when this returns
int run_rows(pcoa_ctx* c, const uint32_t* bits_dev, int64_t nv, int64_t ld, double* out, int out_is_device) {
  if (out_is_device) return launch_rows(c, bits_dev, nv, ld, out);
  const int64_t cap = std::min(nv, kLoadingsOutRows);
  int rc = ensure(c, &c->ld_out, &c->ld_out_cap, cap * c->ld_num_pc);
  if (rc != PCOA_OK) return rc;
  for (int64_t v0 = 0; v0 < nv; v0 += cap) {
    const int64_t rows = std::min(cap, nv - v0);
    if ((rc = launch_rows(c, bits_dev + v0 * ld, rows, ld, c->ld_out)) != PCOA_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(out + v0 * c->ld_num_pc, c->ld_out, sizeof(double) * (size_t)(rows * c->ld_num_pc),
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // c->ld_out is rewritten by the next chunk
  }
  return PCOA_OK;
}

int check_rows_call(pcoa_ctx* c, const char* call, const void* rows, int64_t n_variants, const double* out) {
  if (!c->ld_active) return not_begun(c, call);
  if (n_variants < 0 || (n_variants > 0 && (!rows || !out)))
    return fail(c, PCOA_ERR_INVALID_ARG, std::string(call) + ": the rows or out is NULL, or n_variants < 0");
  return PCOA_OK;
}

}  // namespace

namespace pcoa {

void loadings_destroy(pcoa_ctx* c) {
  for (void* p : {(void*)c->ld_u, (void*)c->ld_bits, (void*)c->ld_out})
    if (p) dev_free(p);
  c->ld_u = nullptr;
  c->ld_bits = nullptr;
  c->ld_out = nullptr;
  c->ld_div = nullptr;
  c->ld_u_cap = c->ld_bits_cap = c->ld_out_cap = 0;
  c->ld_active = false;
}

}  // namespace pcoa

extern "C" {

int pcoa_loadings_begin(pcoa_ctx* c, int32_t num_pc, const double* components, const double* eigenvalues, uint32_t flags) {
  CHECK_CTX(c);
  NOT_ON_GRM(c, "pcoa_loadings_begin");
  if (num_pc <= 0 || num_pc > c->n)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_loadings_begin: num_pc = " + std::to_string(num_pc) + " is outside (0, n_samples]");
  if (!components) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_loadings_begin: components is NULL");
  if (flags & ~(uint32_t)(PCOA_LOADINGS_CENTRE | PCOA_LOADINGS_UNIT))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_loadings_begin: unknown PCOA_LOADINGS_* flag");
  const bool unit = (flags & PCOA_LOADINGS_UNIT) != 0, centre = (flags & PCOA_LOADINGS_CENTRE) != 0;
  if (unit) {
    if (!eigenvalues) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_loadings_begin: PCOA_LOADINGS_UNIT without eigenvalues");
    for (int32_t k = 0; k < num_pc; ++k)
      if (!std::isfinite(eigenvalues[k]) || !(eigenvalues[k] > 0.0))
        return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_loadings_begin: PCOA_LOADINGS_UNIT with eigenvalue " + std::to_string(k) + " = " +
                                                 std::to_string(eigenvalues[k]) + ", which is not a finite positive number");
  }
  const int64_t n = c->n, npad = words_of(c) * 32;
  std::vector<double> prep((size_t)(npad * num_pc + num_pc), 0.0);
  for (int32_t k = 0; k < num_pc; ++k) {
    const double* u = components + (int64_t)k * n;
    double mean = 0.0;
    if (centre) {
      double s = 0.0;
      for (int64_t i = 0; i < n; ++i) s += u[i];   // left to right: the mean is a function of the vector alone
      mean = s / (double)n;
    }
    double* d = prep.data() + (int64_t)k * npad;
    for (int64_t i = 0; i < n; ++i) d[i] = centre ? u[i] - mean : u[i];
    prep[(size_t)(npad * num_pc + k)] = unit ? std::sqrt(eigenvalues[k]) : 1.0;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // kernels of an earlier begin may still read the vectors
  c->ld_active = false;
  int rc = ensure(c, &c->ld_u, &c->ld_u_cap, (int64_t)prep.size());
  if (rc != PCOA_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->ld_u, prep.data(), sizeof(double) * prep.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // `prep` dies here
  c->ld_num_pc = num_pc;
  c->ld_div = unit ? c->ld_u + npad * num_pc : nullptr;
  c->ld_active = true;
  return PCOA_OK;
}

int pcoa_loadings_end(pcoa_ctx* c) {
  CHECK_CTX(c);
  if (!c->ld_active) return PCOA_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // queued loadings kernels read the vectors
  if (c->ld_u) dev_free(c->ld_u);
  c->ld_u = nullptr;
  c->ld_u_cap = 0;
  c->ld_div = nullptr;
  c->ld_num_pc = 0;
  c->ld_active = false;
  return PCOA_OK;
}

int pcoa_loadings_bits(pcoa_ctx* c, const uint32_t* bits, int64_t n_variants, int64_t ld_words, int is_device_ptr, double* out,
                       int out_is_device) {
  CHECK_CTX(c);
  int rc = check_rows_call(c, "pcoa_loadings_bits", bits, n_variants, out);
  if (rc != PCOA_OK) return rc;
  if ((rc = check_ld_words(c, "pcoa_loadings_bits: ", ld_words)) != PCOA_OK) return rc;
  if (n_variants == 0) return PCOA_OK;
  if (is_device_ptr) return run_rows(c, bits, n_variants, ld_words, out, out_is_device);
  // host rows: the copy of one chunk beside the kernels of the chunk before; the caller's rows have been read on return
  const int64_t slot_rows = std::min<int64_t>(kLoadingsSlotRows, std::max<int64_t>(1, ((int64_t)256 << 20) / (words_of(c) * 4)));
  return feed_bits(c, bits, n_variants, ld_words, std::min(n_variants, slot_rows), false, true,
                   [&](const uint32_t* stage, int64_t ld, int64_t v0, int64_t rows) {
                     return run_rows(c, stage, rows, ld, out + v0 * c->ld_num_pc, out_is_device);
                   });
}

int pcoa_loadings_plink_bed(pcoa_ctx* c, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes, int ref_is_a1,
                            int is_device_ptr, double* out, int out_is_device) {
  CHECK_CTX(c);
  int rc = check_rows_call(c, "pcoa_loadings_plink_bed", bed_rows, n_variants, out);
  if (rc != PCOA_OK) return rc;
  if ((rc = check_row_bytes(c, "pcoa_loadings_plink_bed: ", row_bytes)) != PCOA_OK) return rc;
  if ((rc = check_bed_source(c, "pcoa_loadings_plink_bed: ", is_device_ptr, false)) != PCOA_OK) return rc;
  if (n_variants == 0) return PCOA_OK;
  const int64_t words = words_of(c);
  const int64_t slot_rows = std::min<int64_t>(kLoadingsSlotRows, std::max<int64_t>(1, ((int64_t)256 << 20) / row_bytes));
  const int64_t rows_cap = std::min(n_variants, slot_rows);
  if ((rc = ensure(c, &c->ld_bits, &c->ld_bits_cap, rows_cap * words)) != PCOA_OK) return rc;
  return feed_bed(c, bed_rows, n_variants, row_bytes, rows_cap, is_device_ptr, true, bed_decoder(c, row_bytes, ref_is_a1, c->ld_bits),
                  [&](int64_t v0, int64_t rows) { return run_rows(c, c->ld_bits, rows, words, out + v0 * c->ld_num_pc, out_is_device); });
}

int pcoa_loadings_operator(pcoa_ctx* c, int64_t first_variant, int64_t n_variants, double* out, int out_is_device) {
  CHECK_CTX(c);
  if (!c->is_operator) return fail(c, PCOA_ERR_STATE, "pcoa_loadings_operator: not an operator ctx (pcoa_create_operator)");
  if (!c->ld_active) return not_begun(c, "pcoa_loadings_operator");
  if (first_variant < 0 || n_variants < 0 || first_variant > c->op_variants || n_variants > c->op_variants - first_variant)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_loadings_operator: rows [" + std::to_string(first_variant) + ", " +
                                             std::to_string(first_variant + n_variants) + ") are not inside the store's [0, " +
                                             std::to_string(c->op_variants) + ")");
  if (n_variants > 0 && !out) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_loadings_operator: out is NULL");
  const int64_t pitch = operator_pitch_words(c->n), last = first_variant + n_variants;
  int64_t seg0 = 0;   // index in the store of the segment's first row
  for (const auto& s : c->op_segs) {
    const int64_t a = std::max(first_variant, seg0), b = std::min(last, seg0 + s.rows);
    if (a < b) {
      const int rc = run_rows(c, s.p + (a - seg0) * pitch, b - a, pitch, out + (a - first_variant) * c->ld_num_pc, out_is_device);
      if (rc != PCOA_OK) return rc;
    }
    seg0 += s.rows;
  }
  return PCOA_OK;
}

int pcoa_get_loadings_stats(pcoa_ctx* c, pcoa_loadings_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_loadings_stats full;
  std::memset(&full, 0, sizeof(full));
  full.loadings_variants = c->ld_variants;
  full.loadings_bytes = c->ld_bytes;
  full.loadings_seconds = c->tsec[T_LOADINGS];
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
