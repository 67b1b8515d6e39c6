// capi_grm_lsq.hip -- the least-squares projection of sparsely called study samples onto the axes of K (the rule
// is stated at pcoa_grm_project_lsq in pcoa.h, the kernels are grm_lsq.hip's).  pcoa_grm_project places a sample called at a
// share f of the used variants at about f times its position; here every study sample gets the normal equations H_q x = P_q of
// the fit over the variants IT is called at.  t and P come from the kernels of grm_multi.hip exactly as pcoa_grm_project runs
// them (P is its numerator, not divided); H takes one pass over the study's store per chunk of four pairs.  Nothing here writes
// either store; everything runs on the panel's stream, behind whatever the study's stream still holds.
#include <algorithm>
#include <cstring>
#include <string>

#include "pcoa_ctx.h"

using namespace pcoa;

extern "C" {

int pcoa_grm_project_lsq(pcoa_ctx* panel, pcoa_ctx* study, int32_t num_pc, const double* components, double* out_coords,
                         int32_t* out_called, int32_t* out_determined, double* out_normal) {
  CHECK_CTX(panel);
  if (!study) return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_project_lsq: study is NULL");
  if (!panel->is_grm || panel->is_grm_study)
    return fail(panel, PCOA_ERR_STATE, "pcoa_grm_project_lsq: panel is not a GRM ctx with weights of its own (pcoa_create_grm)");
  if (!study->is_grm)
    return fail(panel, PCOA_ERR_STATE, "pcoa_grm_project_lsq: study is not a GRM ctx (pcoa_create_grm_study or pcoa_create_grm)");
  if (study->device != panel->device)
    return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_project_lsq: study sits on device " + std::to_string(study->device) +
                                                 ", the panel on device " + std::to_string(panel->device));
  if (!out_coords) return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_project_lsq: out_coords is NULL");
  if (study->op_variants != panel->op_variants)
    return fail(panel, PCOA_ERR_STATE, "pcoa_grm_project_lsq: the study's store holds " + std::to_string(study->op_variants) +
                                           " variants, the panel's " + std::to_string(panel->op_variants) +
                                           ": both must hold the same variants in the same order");
  if (num_pc < 1 || num_pc > kGrmLsqMaxPc)
    return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_project_lsq: num_pc = " + std::to_string(num_pc) + " is outside [1, " +
                                                 std::to_string(kGrmLsqMaxPc) + "]");
  if (!components) return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_project_lsq: components is NULL");
  int rc = check_device_flags(panel);
  if (rc != PCOA_OK) return rc;
  GrmParams g;
  int64_t used = 0;
  if ((rc = grm_resident_params(panel, &g, &used)) != PCOA_OK) return rc;
  if (used == 0)
    return fail(panel, PCOA_ERR_INVALID_ARG, "pcoa_grm_project_lsq: none of the " + std::to_string(panel->op_variants) +
                                                 " variants in the panel's store is used (M' = 0): K is undefined");
  if (study != panel) {
    if ((rc = check_device_flags(study)) != PCOA_OK) return fail(panel, rc, "pcoa_grm_project_lsq: study: " + study->last_error);
    HIP_TRY(panel, hipStreamSynchronize(study->stream));   // its rows are in place before the panel's stream reads them
  }
  // behind the shared front: ypart [2][ranges][pitch * 16] (the called count's int32 partials use the same memory) | prod [4][V]
  // | hpart [4][ranges][pitch * 16] | normal [pairs + P][Nq] (the solve leaves the coordinates where P was) | called [Nq],
  // determined [Nq], the undetermined count: int32
  const int64_t v = panel->op_variants, nq = study->n, ystride = (int64_t)grm_pitch_words(study->n) * 16;
  const int64_t ranges = grm_store_ranges(study), cstride = ranges * ystride;
  const int32_t pairs = num_pc * (num_pc + 1) / 2;
  GrmMultiWs w;
  if ((rc = grm_multi_ws(panel, num_pc,
                         (2 + kGrmLsqMaxChunk) * cstride + kGrmLsqMaxChunk * v + (int64_t)(pairs + num_pc) * nq + nq + 1, &w)) != PCOA_OK)
    return rc;
  double* const ypart = w.rest;
  double* const prod = ypart + 2 * cstride;
  double* const hpart = prod + kGrmLsqMaxChunk * v;
  double* const normal = hpart + kGrmLsqMaxChunk * cstride;
  double* const coords = normal + (int64_t)pairs * nq;
  int32_t* const called = reinterpret_cast<int32_t*>(coords + (int64_t)num_pc * nq);
  int32_t* const determined = called + nq;
  int32_t* const undetermined = determined + nq;
  if ((rc = grm_panel_t(panel, g, w, num_pc, components, nullptr)) != PCOA_OK) return rc;
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
      HIP_TRY(panel, launch_grm_lsq_finish(ypart, (int32_t)ranges, cstride, study->n, k, coords + (int64_t)c0 * nq, panel->stream));
      c0 += k;
    }
  }
  {
    ScopedTimer timer(panel, T_GRM_LSQ_PAIRS);
    for (int32_t e0 = 0; e0 < pairs;) {
      const int32_t j = grm_lsq_chunk(pairs - e0);
      HIP_TRY(panel, launch_grm_lsq_products(w.t, v, g.d, g.used, v, e0, j, prod, panel->stream));
      int64_t row0 = 0, q0 = 0;
      for (const auto& sg : study->op_segs) {
        HIP_TRY(panel, launch_grm_lsq_pairs(sg.p, (int32_t)sg.rows, study->n, prod + row0, v, j, hpart + q0 * ystride, cstride,
                                            panel->stream));
        row0 += sg.rows;
        q0 += (sg.rows + kGrmRangeRows - 1) / kGrmRangeRows;
      }
      HIP_TRY(panel, launch_grm_lsq_finish(hpart, (int32_t)ranges, cstride, study->n, j, normal + (int64_t)e0 * nq, panel->stream));
      e0 += j;
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
  if (out_normal)   // before the solve overwrites it
    HIP_TRY(panel, hipMemcpyAsync(out_normal, normal, sizeof(double) * (size_t)(pairs + num_pc) * (size_t)nq, hipMemcpyDeviceToHost,
                                  panel->stream));
  HIP_TRY(panel, hipMemsetAsync(undetermined, 0, sizeof(int32_t), panel->stream));
  {
    ScopedTimer timer(panel, T_GRM_LSQ_SOLVE);
    HIP_TRY(panel, launch_grm_lsq_solve(normal, study->n, num_pc, determined, undetermined, panel->stream));
  }
  HIP_TRY(panel, hipMemcpyAsync(out_coords, coords, sizeof(double) * (size_t)num_pc * (size_t)nq, hipMemcpyDeviceToHost, panel->stream));
  if (out_determined)
    HIP_TRY(panel, hipMemcpyAsync(out_determined, determined, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, panel->stream));
  HIP_TRY(panel, hipMemcpyAsync(&panel->hw->lsq, undetermined, sizeof(int32_t), hipMemcpyDeviceToHost, panel->stream));
  HIP_TRY(panel, hipStreamSynchronize(panel->stream));
  panel->grm_lsq_calls += 1;
  panel->grm_lsq_pair_vectors += pairs;
  panel->grm_lsq_undetermined = panel->hw->lsq;
  return PCOA_OK;
}

int pcoa_get_grm_lsq_stats(pcoa_ctx* c, pcoa_grm_lsq_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(double)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  const int rc = fp4_sync_point(c);
  if (rc != PCOA_OK) return rc;
  drain_events(c, true);
  pcoa_grm_lsq_stats full;
  std::memset(&full, 0, sizeof(full));
  full.grm_lsq_calls = c->grm_lsq_calls;
  full.grm_lsq_pair_vectors = c->grm_lsq_pair_vectors;
  full.grm_lsq_pairs_seconds = c->tsec[T_GRM_LSQ_PAIRS];
  full.grm_lsq_solve_seconds = c->tsec[T_GRM_LSQ_SOLVE];
  full.grm_lsq_undetermined = c->grm_lsq_undetermined;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
