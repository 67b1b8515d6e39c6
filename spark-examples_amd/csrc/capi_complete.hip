// capi_complete.hip -- the pairwise-complete similarity (the kernels and the rule: complete.hip).
// pcoa_set_call_companion binds a second ordinary engine, the companion, whose S is Q, the Gram matrix of the missing-call
// bitsets; from then on pcoa_compute, pcoa_center_read_f64 and pcoa_debug_centred_matvec centre and decompose
// K(i, j) = S(i, j) / M(i, j), M the number of variants at which both samples were called.  Like the measure, the binding
// says how the ctx DECOMPOSES S, not how it accumulates it: S, the reductions, the reads and the screen never look at it.
// pcoa_accumulate_plink_bed_calls feeds both engines from one read of the raw .bed rows, through the row feed (row_feed.h).
#include <string>

#include "pcoa_ctx.h"
#include "row_feed.h"

using namespace pcoa;

namespace pcoa {

void complete_bind(const pcoa_ctx* c, EigWorkspace* ws) {
  ws->measure = PCOA_SIMILARITY_SHARED;
  ws->comp_q32 = c->companion->s32;
  ws->comp_c = c->complete_c;
  ws->comp_v = c->companion_v;
}

int complete_b(pcoa_ctx* c, double* b) {
  HIP_TRY(c, launch_complete_center(c->s32, c->s64, c->companion->s32, c->n, c->complete_c, c->companion_v, c->colmean, c->stats,
                                    b, c->stream));
  return PCOA_OK;
}

// The centring of the rule from the current S and the current Q.  The companion is finalized and its input checks are read
// first (that synchronises its stream: everything it was fed is in Q before a kernel of c's stream reads it); its errors are
// reported on c.
int complete_centre(pcoa_ctx* c, bool sym_form, double* b) {
  pcoa_ctx* q = c->companion;
  const int32_t n = c->n;
  int rc = finalize_impl(q);
  if (rc == PCOA_OK) rc = check_device_flags(q);
  if (rc != PCOA_OK) return fail(c, rc, "the call companion: " + q->last_error);
  if (q->s64)
    return fail(c, PCOA_ERR_STATE, "the call companion has an int64 part (more than 2^30 variants accumulated into it): the "
                                   "pairwise-complete similarity over an int64 Q is not built");
  if (!c->complete_c) HIP_TRY(c, dev_alloc((void**)&c->complete_c, sizeof(int64_t) * ((size_t)n + 2), c->device));
  int32_t* flag = reinterpret_cast<int32_t*>(c->complete_c + n);
  const int64_t v = c->companion_v;
  HIP_TRY(c, launch_complete_diag(q->s32, n, v, c->complete_c, flag, c->stream));
  double* ones = c->ws.q;   // an N-vector of the eigensolver workspace: free until the solver starts
  if (sym_form)
    HIP_TRY(c, launch_complete_row_sums_sym(c->s32, q->s32, n, c->complete_c, v, ones, c->sym_part, c->row_sums, c->stream));
  else
    HIP_TRY(c, launch_complete_row_sums(c->s32, c->s64, q->s32, n, c->complete_c, v, ones, c->row_sums, c->stream));
  HIP_TRY(c, launch_measure_stats(c->row_sums, n, c->stats, c->nz, c->stream));
  HIP_TRY(c, launch_col_means(c->row_sums, n, c->colmean, c->stream));
  if (b && (rc = complete_b(c, b)) != PCOA_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(&c->hw->cflag, flag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->hw->cflag)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_set_call_companion: n_variants is smaller than a sample's missing count (n_variants = " +
                                         std::to_string(v) + ", below a diagonal entry of the companion's S)");
  return PCOA_OK;
}

// the binding, and the companion with it where the ctx owns it (a subset's)
static void drop_companion(pcoa_ctx* c) {
  if (c->companion && c->companion_owned) {
    pcoa_destroy(c->companion);
    (void)hipSetDevice(c->device);
  }
  c->companion = nullptr;
  c->companion_owned = false;
  c->companion_v = 0;
}

void complete_destroy(pcoa_ctx* c) {
  if (c->complete_c) dev_free(c->complete_c);
  if (c->calls_bits) dev_free(c->calls_bits);
  if (c->calls_decoded) (void)hipEventDestroy(c->calls_decoded);
  if (c->calls_read) (void)hipEventDestroy(c->calls_read);
  c->complete_c = nullptr;
  c->calls_bits = nullptr;
  c->calls_decoded = c->calls_read = nullptr;
  drop_companion(c);
}

}  // namespace pcoa

namespace {

const char* engine_kind(const pcoa_ctx* c) { return c->is_operator ? "an operator ctx (pcoa_create_operator)" : "a strip owner (pcoa_create_strip)"; }

}  // namespace

extern "C" {

int pcoa_set_call_companion(pcoa_ctx* c, pcoa_ctx* missing, int64_t n_variants) {
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_set_call_companion: ctx is NULL");
  if (!missing) {   // unbind (a companion the ctx owns -- a subset's -- goes with the binding)
    drop_companion(c);
    return PCOA_OK;
  }
  if (missing == c) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_set_call_companion: missing is ctx itself");
  NOT_ON_GRM(c, "pcoa_set_call_companion");
  if (missing->n != c->n)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_set_call_companion: the companion has N = " + std::to_string(missing->n) +
                                         " samples, ctx has " + std::to_string(c->n));
  if (n_variants < 0) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_set_call_companion: n_variants < 0");
  if (c->is_operator || c->is_strip)
    return fail(c, PCOA_ERR_STATE, std::string("pcoa_set_call_companion: ctx is ") + engine_kind(c) +
                                       ", which holds no full S; use a full engine (pcoa_create)");
  if (missing->is_operator || missing->is_strip)
    return fail(c, PCOA_ERR_STATE, std::string("pcoa_set_call_companion: the companion is ") + engine_kind(missing) +
                                       ", which holds no full S; use a full engine (pcoa_create)");
  if (missing->device != c->device)
    return fail(c, PCOA_ERR_STATE, "pcoa_set_call_companion: the companion is on device " + std::to_string(missing->device) +
                                       ", ctx on device " + std::to_string(c->device) + ": different devices");
  if (missing->companion)
    return fail(c, PCOA_ERR_STATE, "pcoa_set_call_companion: the companion itself has a companion bound");
  if (c->similarity != PCOA_SIMILARITY_SHARED)
    return fail(c, PCOA_ERR_STATE, "pcoa_set_call_companion: ctx decomposes a Jaccard / cosine measure (pcoa_set_similarity); the "
                                   "pairwise-complete form of a measure is not built");
  if (c->companion != missing) drop_companion(c);
  c->companion = missing;
  c->companion_v = n_variants;
  return PCOA_OK;
}

int pcoa_get_call_companion(const pcoa_ctx* c, pcoa_ctx** missing_out, int64_t* n_variants_out) {
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_get_call_companion: ctx is NULL");
  if (missing_out) *missing_out = c->companion;
  if (n_variants_out) *n_variants_out = c->companion ? c->companion_v : 0;
  return PCOA_OK;
}

// pcoa_accumulate_plink_bed through the same row feed (row_feed.h) with the pair decode: the raw rows cross the link once, one
// kernel reads them once and writes the carrier rows (c->tile) and the missing rows (c->calls_bits).  The carrier rows go into c
// on its stream, the missing rows into the companion on ITS stream:
//   calls_decoded  recorded on c's stream behind the decode; the companion's stream waits for it before its pre-pass
//   calls_read     recorded on the companion's stream behind that pre-pass; c's stream waits for it before the next decode
//                  rewrites calls_bits (in this call or a later one)
// No host wait beyond the existing call's.
int pcoa_accumulate_plink_bed_calls(pcoa_ctx* c, pcoa_ctx* missing, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes,
                                    int ref_is_a1, int is_device_ptr) {
  CHECK_CTX(c);
  const char* fn = "pcoa_accumulate_plink_bed_calls: ";
  if (!missing) return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "missing is NULL");
  if (missing == c) return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "missing is ctx itself");
  NOT_ON_GRM(c, "pcoa_accumulate_plink_bed_calls");
  if (missing->n != c->n) return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "the companion's N differs from ctx's");
  if (missing->is_operator || missing->is_strip || !missing->use_i8 || missing->device != c->device)
    return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "the companion must be an ordinary packed-operand full engine "
                                                           "(pcoa_create, not PCOA_FLAG_GRAM_F32_MFMA) on ctx's device");
  if (n_variants < 0 || (n_variants > 0 && !bed_rows)) return fail(c, PCOA_ERR_INVALID_ARG, "bed_rows is NULL or n_variants < 0");
  int rc = check_row_bytes(c, "", row_bytes);
  if (rc != PCOA_OK) return rc;
  if (!c->use_i8)
    return fail(c, PCOA_ERR_INVALID_ARG, "the PLINK boundary needs a packed-operand engine (not PCOA_FLAG_GRAM_F32_MFMA)");
  if ((rc = check_bed_source(c, "", is_device_ptr, true)) != PCOA_OK) return rc;
  if (n_variants == 0) return PCOA_OK;
  const int64_t words = words_of(c);
  const int64_t rows_cap = std::min<int64_t>(n_variants, (int64_t)1 << 17);
  if (c->calls_read_pending && rows_cap * words > c->calls_bits_cap) {   // the buffer is about to be replaced: its reader first
    HIP_TRY(c, hipEventSynchronize(c->calls_read));
    c->calls_read_pending = false;
  }
  rc = ensure(c, &c->tile, &c->tile_elems, rows_cap * words);
  if (rc == PCOA_OK) rc = ensure(c, &c->calls_bits, &c->calls_bits_cap, rows_cap * words);
  if (rc != PCOA_OK) return rc;
  if (!c->calls_decoded) HIP_TRY(c, hipEventCreateWithFlags(&c->calls_decoded, hipEventDisableTiming));
  if (!c->calls_read) HIP_TRY(c, hipEventCreateWithFlags(&c->calls_read, hipEventDisableTiming));
  uint32_t* bits = reinterpret_cast<uint32_t*>(c->tile);
  return feed_bed(
      c, bed_rows, n_variants, row_bytes, rows_cap, is_device_ptr, true,
      [&](const uint8_t* src, int64_t, int64_t rows) -> int {
        if (c->calls_read_pending) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->calls_read, 0));
        {
          ScopedTimer t(c, T_DENSIFY);
          HIP_TRY(c, launch_plink_bed_to_bits_pair(src, row_bytes, rows, c->n, words, ref_is_a1 ? 1 : 0, bits, c->calls_bits, c->stream));
        }
        HIP_TRY(c, hipEventRecord(c->calls_decoded, c->stream));
        return PCOA_OK;
      },
      [&](int64_t, int64_t rows) -> int {
        int rc2 = gram_device_bits(c, bits, rows, words, false);
        if (rc2 != PCOA_OK) return rc2;
        HIP_TRY(c, hipStreamWaitEvent(missing->stream, c->calls_decoded, 0));
        if ((rc2 = gram_device_bits(missing, c->calls_bits, rows, words, false)) != PCOA_OK)
          return fail(c, rc2, std::string(fn) + "the companion: " + missing->last_error);
        HIP_TRY(c, hipEventRecord(c->calls_read, missing->stream));
        c->calls_read_pending = true;
        return PCOA_OK;
      });
}

}  // extern "C"
