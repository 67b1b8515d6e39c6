// capi_measure.hip -- pcoa_set_similarity / pcoa_get_similarity, and the centring of a Jaccard or cosine measure that
// pcoa_compute, pcoa_center_read_f64 and pcoa_debug_centred_matvec run in place of launch_center when one is set (DESIGN.md
// 4.11; the kernels and the rule: measure.hip).  The measure says how the ctx DECOMPOSES S, not how it accumulates it: S, its
// int64 part, the reductions, the reads and the screen never look at it.
#include <string>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace pcoa {

void measure_bind(const pcoa_ctx* c, EigWorkspace* ws) {
  if (c->companion) return complete_bind(c, ws);
  ws->measure = c->similarity;
  ws->diag = c->measure_diag;
  ws->qcos = c->measure_q;
}

int measure_b(pcoa_ctx* c, double* b) {
  if (c->companion) return complete_b(c, b);
  HIP_TRY(c, launch_measure_center(c->s32, c->s64, c->n, c->similarity, c->measure_diag, c->measure_q, c->colmean, c->stats, b,
                                   c->stream));
  return PCOA_OK;
}

int measure_centre(pcoa_ctx* c, bool sym_form, double* b) {
  if (c->companion) return complete_centre(c, sym_form, b);
  const int32_t n = c->n;
  if (!c->measure_diag) HIP_TRY(c, dev_alloc((void**)&c->measure_diag, sizeof(int64_t) * (size_t)n, c->device));
  if (c->similarity == PCOA_SIMILARITY_COSINE && !c->measure_q)
    HIP_TRY(c, dev_alloc((void**)&c->measure_q, sizeof(double) * (size_t)n, c->device));
  HIP_TRY(c, launch_measure_diag(c->s32, c->s64, n, c->similarity, c->measure_diag, c->measure_q, c->stream));
  double* ones = c->ws.q;   // an N-vector of the eigensolver workspace: free until the solver starts
  if (sym_form)
    HIP_TRY(c, launch_measure_row_sums_sym(c->s32, n, c->similarity, c->measure_diag, c->measure_q, ones, c->sym_part, c->row_sums,
                                           c->stream));
  else
    HIP_TRY(c, launch_measure_row_sums(c->s32, c->s64, n, c->similarity, c->measure_diag, c->measure_q, ones, c->row_sums, c->stream));
  HIP_TRY(c, launch_measure_stats(c->row_sums, n, c->stats, c->nz, c->stream));
  HIP_TRY(c, launch_col_means(c->row_sums, n, c->colmean, c->stream));
  return b ? measure_b(c, b) : PCOA_OK;
}

}  // namespace pcoa

extern "C" {

int pcoa_set_similarity(pcoa_ctx* c, int32_t kind) {
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_set_similarity: ctx is NULL");
  if (kind != PCOA_SIMILARITY_SHARED && kind != PCOA_SIMILARITY_JACCARD && kind != PCOA_SIMILARITY_COSINE)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_set_similarity: kind = " + std::to_string(kind) +
                                         " is none of PCOA_SIMILARITY_SHARED, _JACCARD, _COSINE");
  if (kind != PCOA_SIMILARITY_SHARED) {
    NOT_ON_GRM(c, "pcoa_set_similarity");
    if (c->is_operator)
      return fail(c, PCOA_ERR_STATE, "pcoa_set_similarity: an operator ctx (pcoa_create_operator) holds the carrier bitsets, not S: "
                                     "a measure over the implicit operator is not built; use a full engine (pcoa_create)");
    if (c->is_strip)
      return fail(c, PCOA_ERR_STATE, "pcoa_set_similarity: a strip owner holds N x cols of S, not the diagonal of every sample: a "
                                     "measure over strips is not built; use a full engine (pcoa_create)");
    if (c->companion)
      return fail(c, PCOA_ERR_STATE, "pcoa_set_similarity: a call companion is bound (pcoa_set_call_companion): a Jaccard / cosine "
                                     "measure of the pairwise-complete similarity is not built; unbind the companion first");
  }
  c->similarity = kind;
  return PCOA_OK;
}

int pcoa_get_similarity(const pcoa_ctx* c, int32_t* kind_out) {
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_get_similarity: ctx is NULL");
  if (!kind_out) return fail(const_cast<pcoa_ctx*>(c), PCOA_ERR_INVALID_ARG, "pcoa_get_similarity: kind_out is NULL");
  *kind_out = c->similarity;
  return PCOA_OK;
}

}  // extern "C"
