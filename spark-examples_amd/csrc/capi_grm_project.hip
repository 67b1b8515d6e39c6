// capi_grm_project.hip -- SNP weights of the axes of K and the projection of new samples onto them.  With
// K = A^T D A / M', K u_c = lambda_c u_c: t_c = D A u_c is pass 1 of the product applied to u_c (over the PANEL's rows), the
// left singular vectors of Z = D^1/2 A / sqrt(M') are w_c = t_c / sqrt(d M' lambda_c), and a sample q genotyped at the same
// variants lands at (sum_v g_vq t_vc + sum_v c_vq s_vc) / M' / lambda_c, s_c = -(mu t_c): pass 2 over the STUDY's rows with the
// panel's mu, d and M'.  Both passes run for two components at a time (grm_multi.hip); every column has the bits of a one-vector
// run.  Nothing here writes either store; everything runs on the panel's stream, behind whatever the study's stream still holds.
#include <algorithm>
#include <cmath>
#include <string>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace {

// what both calls ask of the panel and of the axes; on success the panel's parameters are resident and M' > 0
int check_panel(pcoa_ctx* panel, const char* call, int32_t num_pc, const double* components, const double* eigenvalues, GrmParams* g,
                int64_t* used) {
  const std::string fn = std::string(call) + ": ";
  if (!panel->is_grm || panel->is_grm_study)
    return fail(panel, PCOA_ERR_STATE, fn + "panel is not a GRM ctx with weights of its own (pcoa_create_grm)");
  if (num_pc < 1) return fail(panel, PCOA_ERR_INVALID_ARG, fn + "num_pc = " + std::to_string(num_pc) + " must be at least 1");
  if (!components || !eigenvalues) return fail(panel, PCOA_ERR_INVALID_ARG, fn + "components or eigenvalues is NULL");
  for (int32_t c = 0; c < num_pc; ++c)
    if (!(eigenvalues[c] > 0.0) || !std::isfinite(eigenvalues[c]))
      return fail(panel, PCOA_ERR_INVALID_ARG, fn + "eigenvalue " + std::to_string(c) + " = " + std::to_string(eigenvalues[c]) +
                                                   " is not positive and finite");
  int rc = check_device_flags(panel);
  if (rc != PCOA_OK) return rc;
  if ((rc = grm_resident_params(panel, g, used)) != PCOA_OK) return rc;
  if (*used == 0)
    return fail(panel, PCOA_ERR_INVALID_ARG, fn + "none of the " + std::to_string(panel->op_variants) +
                                                 " variants in the panel's store is used (M' = 0): K is undefined");
  return PCOA_OK;
}

}  // namespace

namespace pcoa {

int grm_multi_ws(pcoa_ctx* panel, int32_t num_pc, int64_t rest_doubles, GrmMultiWs* w) {
  const int64_t n = panel->n, v = panel->op_variants, groups = grm_groups(panel->n), p = num_pc;
  const int64_t need = p * n + p + 2 * p * v + 2 * groups * v + rest_doubles;
  const int rc = ensure(panel, &panel->grm_mw, &panel->grm_mw_cap, need);
  if (rc != PCOA_OK) return rc;
  w->u = panel->grm_mw;
  w->lam = w->u + p * n;
  w->t = w->lam + p;
  w->s = w->t + p * v;
  w->tpart = w->s + p * v;
  w->rest = w->tpart + 2 * groups * v;
  return PCOA_OK;
}

int grm_panel_t(pcoa_ctx* panel, const GrmParams& g, const GrmMultiWs& w, int32_t num_pc, const double* components,
                const double* eigenvalues) {
  const int64_t n = panel->n, v = panel->op_variants, groups = grm_groups(panel->n);
  HIP_TRY(panel, hipMemcpyAsync(w.u, components, sizeof(double) * (size_t)num_pc * (size_t)n, hipMemcpyHostToDevice, panel->stream));
  if (eigenvalues)
    HIP_TRY(panel, hipMemcpyAsync(w.lam, eigenvalues, sizeof(double) * (size_t)num_pc, hipMemcpyHostToDevice, panel->stream));
  ScopedTimer timer(panel, T_OPERATOR);
  for (int32_t c0 = 0; c0 < num_pc;) {
    const int32_t k = grm_multi_chunk(num_pc - c0);
    int64_t row0 = 0;
    for (const auto& sg : panel->op_segs) {
      HIP_TRY(panel, launch_grm_ax_multi(sg.p, (int32_t)sg.rows, panel->n, g.mu + row0, w.u + (int64_t)c0 * n, n, k, w.tpart + row0, v,
                                         groups * v, panel->stream));
      row0 += sg.rows;
    }
    for (int32_t c = 0; c < k; ++c)
      HIP_TRY(panel, launch_grm_combine_t(w.tpart + (int64_t)c * groups * v, v, panel->n, v, g.mu, g.d, w.t + (int64_t)(c0 + c) * v,
                                          w.s + (int64_t)(c0 + c) * v, panel->stream));
    c0 += k;
  }
  return PCOA_OK;
}

}  // namespace pcoa

extern "C" {

int pcoa_create_grm_study(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags) {
  return create_grm_study_engine(out, n_samples, device_ordinal, flags);
}

int pcoa_grm_weights(pcoa_ctx* panel, int32_t num_pc, const double* components, const double* eigenvalues, int32_t scaled,
                     int64_t first_variant, int64_t n_variants, double* out) {
  CHECK_CTX(panel);
  GrmParams g;
  int64_t used = 0;
  int rc = check_panel(panel, "pcoa_grm_weights", num_pc, components, eigenvalues, &g, &used);
  if (rc != PCOA_OK) return rc;
  const int64_t v = panel->op_variants;
  if (first_variant < 0 || n_variants < 0 || first_variant > v || n_variants > v - first_variant)
    return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_weights: rows [" + std::to_string(first_variant) + ", " +
                                                 std::to_string(first_variant + n_variants) + ") are not inside the store's " +
                                                 std::to_string(v));
  if (n_variants > 0 && !out) return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_weights: out is NULL");
  if (n_variants == 0) return PCOA_OK;
  GrmMultiWs w;
  if ((rc = grm_multi_ws(panel, num_pc, n_variants * num_pc, &w)) != PCOA_OK) return rc;
  if ((rc = grm_panel_t(panel, g, w, num_pc, components, eigenvalues)) != PCOA_OK) return rc;
  HIP_TRY(panel, launch_grm_weights_out(w.t, v, g.d, g.used, g.mprime, w.lam, scaled ? 1 : 0, first_variant, n_variants, num_pc, w.rest,
                                        panel->stream));
  HIP_TRY(panel, hipMemcpyAsync(out, w.rest, sizeof(double) * (size_t)n_variants * (size_t)num_pc, hipMemcpyDeviceToHost, panel->stream));
  HIP_TRY(panel, hipStreamSynchronize(panel->stream));
  return PCOA_OK;
}

int pcoa_grm_project(pcoa_ctx* panel, pcoa_ctx* study, int32_t num_pc, const double* components, const double* eigenvalues,
                     double* out_coords, int32_t* out_called) {
  CHECK_CTX(panel);
  if (!study) return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_project: study is NULL");
  if (!panel->is_grm || panel->is_grm_study)
    return fail(panel, PCOA_ERR_STATE, "pcoa_grm_project: panel is not a GRM ctx with weights of its own (pcoa_create_grm)");
  if (!study->is_grm)
    return fail(panel, PCOA_ERR_STATE, "pcoa_grm_project: study is not a GRM ctx (pcoa_create_grm_study or pcoa_create_grm)");
  if (study->device != panel->device)
    return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_project: study sits on device " + std::to_string(study->device) +
                                                 ", the panel on device " + std::to_string(panel->device));
  if (!out_coords) return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_project: out_coords is NULL");
  if (study->op_variants != panel->op_variants)
    return fail(panel, PCOA_ERR_STATE, "pcoa_grm_project: the study's store holds " + std::to_string(study->op_variants) +
                                           " variants, the panel's " + std::to_string(panel->op_variants) +
                                           ": both must hold the same variants in the same order");
  GrmParams g;
  int64_t used = 0;
  int rc = check_panel(panel, "pcoa_grm_project", num_pc, components, eigenvalues, &g, &used);
  if (rc != PCOA_OK) return rc;
  if (study != panel) {
    if ((rc = check_device_flags(study)) != PCOA_OK) return fail(panel, rc, "pcoa_grm_project: study: " + study->last_error);
    HIP_TRY(panel, hipStreamSynchronize(study->stream));   // its rows are in place before the panel's stream reads them
  }
  // behind the shared front: ypart [2][ranges][pitch * 16] (the called count's int32 partials use the same memory) | coords [P][Nq]
  // | called [Nq] int32
  const int64_t v = panel->op_variants, nq = study->n, ystride = (int64_t)grm_pitch_words(study->n) * 16;
  const int64_t ranges = grm_store_ranges(study), cstride = ranges * ystride;
  GrmMultiWs w;
  if ((rc = grm_multi_ws(panel, num_pc, 2 * cstride + (int64_t)num_pc * nq + (nq + 1) / 2, &w)) != PCOA_OK) return rc;
  double* const ypart = w.rest;
  double* const coords = ypart + 2 * cstride;
  int32_t* const called = reinterpret_cast<int32_t*>(coords + (int64_t)num_pc * nq);
  if ((rc = grm_panel_t(panel, g, w, num_pc, components, eigenvalues)) != PCOA_OK) return rc;
  {
    ScopedTimer timer(panel, T_OPERATOR);
    for (int32_t c0 = 0; c0 < num_pc;) {
      const int32_t k = grm_multi_chunk(num_pc - c0);
      int64_t row0 = 0, q0 = 0;
      for (const auto& sg : study->op_segs) {
        HIP_TRY(panel, launch_grm_at_multi(sg.p, (int32_t)sg.rows, study->n, w.t + (int64_t)c0 * v + row0, w.s + (int64_t)c0 * v + row0, v,
                                           k, ypart + q0 * ystride, cstride, panel->stream));
        row0 += sg.rows;
        q0 += (sg.rows + kGrmRangeRows - 1) / kGrmRangeRows;
      }
      HIP_TRY(panel, launch_grm_project_finish(ypart, (int32_t)ranges, cstride, study->n, k, g.mprime, w.lam + c0,
                                               coords + (int64_t)c0 * nq, panel->stream));
      c0 += k;
    }
  }
  if (out_called) {
    ScopedTimer timer(panel, T_CENTER);
    int32_t* const ipart = reinterpret_cast<int32_t*>(ypart);
    int64_t row0 = 0, q0 = 0;
    for (const auto& sg : study->op_segs) {
      HIP_TRY(panel, launch_grm_called(sg.p, (int32_t)sg.rows, study->n, g.used + row0, ipart + q0 * ystride, panel->stream));
      row0 += sg.rows;
      q0 += (sg.rows + kGrmRangeRows - 1) / kGrmRangeRows;
    }
    HIP_TRY(panel, launch_grm_called_sum(ipart, (int32_t)ranges, study->n, called, panel->stream));
    HIP_TRY(panel, hipMemcpyAsync(out_called, called, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, panel->stream));
  }
  HIP_TRY(panel, hipMemcpyAsync(out_coords, coords, sizeof(double) * (size_t)num_pc * (size_t)nq, hipMemcpyDeviceToHost, panel->stream));
  HIP_TRY(panel, hipStreamSynchronize(panel->stream));
  return PCOA_OK;
}

}  // extern "C"
