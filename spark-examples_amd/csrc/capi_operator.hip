// capi_operator.hip -- the implicit similarity operator of the C ABI (pcoa_create_operator): a ctx that keeps the carrier
// bitsets of every variant and applies S = X^T X to a vector as two passes over them (operator_bits.hip), so that computePca
// needs neither the N^2 V matrix-core work of the Gram nor the 4 N^2 bytes of S.  Here: the bit store (segments that are
// allocated as it grows and never reallocated or copied), the exact row sums and the centring derived from them, the product,
// and computePca as the engine's Lanczos iteration over that product.
#include <algorithm>
#include <string>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace {

int64_t seg_bytes(const pcoa_ctx* c) { return c->op_seg_rows * store_pitch_words(c) * 4; }

// ranges of the second pass over the whole store: every segment is cut into ranges of kOperatorRangeRows rows of its own
int64_t store_ranges(const pcoa_ctx* c) {
  int64_t q = 0;
  for (const auto& s : c->op_segs) q += (s.rows + kOperatorRangeRows - 1) / kOperatorRangeRows;
  return q;
}

// layout of op_ws, in doubles: t [V] | tpart [groups][V] | ypart [ranges][pitch * 32] | dots [8].  The integer passes of the
// row sums use the same memory: the popcounts (int32) in t's place, the int64 partials in ypart's.
struct OpWorkspace {
  double *t, *tpart, *ypart, *dots;
  int64_t vstride, ranges;
};

int ensure_op_ws(pcoa_ctx* c, OpWorkspace* w) {
  const int64_t v = std::max<int64_t>(c->op_variants, 1), groups = operator_groups(c->n);
  const int64_t ranges = std::max<int64_t>(store_ranges(c), 1), ystride = (int64_t)operator_pitch_words(c->n) * 32;
  const int64_t need = v + groups * v + ranges * ystride + 8;
  const int rc = ensure(c, &c->op_ws, &c->op_ws_cap, need);
  if (rc != PCOA_OK) return rc;
  w->t = c->op_ws;
  w->tpart = w->t + v;
  w->ypart = w->tpart + groups * v;
  w->dots = w->ypart + ranges * ystride;
  w->vstride = v;
  w->ranges = store_ranges(c);
  return PCOA_OK;
}

// rowSums (VariantsPca.scala:206) = X^T (X 1), exact: popcount per row, then int64 column sums; from them nonZeroRows, the
// matrix mean and the means rowSums / N (:207-215) with the kernels every other engine uses.  Resident until the store changes.
int operator_centering(pcoa_ctx* c) {
  if (c->op_centering_set) return PCOA_OK;
  int rc = ensure_workspace(c, 1);
  if (rc != PCOA_OK) return rc;
  OpWorkspace w;
  if ((rc = ensure_op_ws(c, &w)) != PCOA_OK) return rc;
  int32_t* cnt = reinterpret_cast<int32_t*>(w.t);
  int64_t* ipart = reinterpret_cast<int64_t*>(w.ypart);
  int64_t* rs_i64 = reinterpret_cast<int64_t*>(c->stats + 2);   // (launch_center's layout: behind stats[0..1])
  const int64_t ystride = (int64_t)operator_pitch_words(c->n) * 32;
  {
    ScopedTimer t(c, T_CENTER);
    int64_t row0 = 0, q0 = 0;
    for (const auto& s : c->op_segs) {
      HIP_TRY(c, launch_operator_popcount(s.p, (int32_t)s.rows, c->n, cnt + row0, c->stream));
      HIP_TRY(c, launch_operator_xt_i64(s.p, (int32_t)s.rows, c->n, cnt + row0, ipart + q0 * ystride, c->stream));
      row0 += s.rows;
      q0 += (s.rows + kOperatorRangeRows - 1) / kOperatorRangeRows;
    }
    HIP_TRY(c, launch_operator_row_sums_finish(ipart, (int32_t)w.ranges, c->n, rs_i64, c->row_sums, c->stream));
    HIP_TRY(c, launch_center(nullptr, nullptr, c->n, c->row_sums, c->stats, c->nz, nullptr, c->stream, true));
    HIP_TRY(c, launch_col_means(c->row_sums, c->n, c->colmean, c->stream));
  }
  c->op_centering_set = true;
  return PCOA_OK;
}

// one product on the ctx stream (queued, not waited for): y = S v, or y = B v with the resident centring
hipError_t operator_product(pcoa_ctx* c, const OpWorkspace& w, const double* v, double* y, int centred) {
  hipError_t e = hipSuccess;
  const int64_t ystride = (int64_t)operator_pitch_words(c->n) * 32;
  if (centred && (e = launch_operator_dots(v, c->colmean, c->n, w.dots, c->stream)) != hipSuccess) return e;
  int64_t row0 = 0;
  for (const auto& s : c->op_segs) {
    if ((e = launch_operator_xv(s.p, (int32_t)s.rows, c->n, v, w.tpart + row0, w.vstride, c->stream)) != hipSuccess) return e;
    row0 += s.rows;
  }
  if ((e = launch_operator_combine_t(w.tpart, w.vstride, c->n, c->op_variants, w.t, c->stream)) != hipSuccess) return e;
  int64_t q0 = 0;
  row0 = 0;
  for (const auto& s : c->op_segs) {
    if ((e = launch_operator_xt_f64(s.p, (int32_t)s.rows, c->n, w.t + row0, w.ypart + q0 * ystride, c->stream)) != hipSuccess) return e;
    row0 += s.rows;
    q0 += (s.rows + kOperatorRangeRows - 1) / kOperatorRangeRows;
  }
  c->op_products += 1;
  return launch_operator_finish(w.ypart, (int32_t)w.ranges, c->n, c->colmean, c->stats, w.dots, centred, y, c->stream);
}

// N < 32 (below the Lanczos path): the resident segments go, as device bitsets, into a temporary full engine on the same
// device, whose pcoa_compute is the full engine's result by construction (the arrangement of pcoa_compute_strips at that N)
int operator_compute_small(pcoa_ctx* c, int32_t num_pc, double* out_components, double* out_eigenvalues, int32_t* out_nonzero_rows) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // the appends have landed
  pcoa_ctx* tmp = nullptr;
  int rc = pcoa_create(&tmp, c->n, c->device, c->flags);
  if (rc != PCOA_OK) return fail(c, rc, std::string("operator compute: temporary engine: ") + pcoa_last_error(nullptr));
  for (const auto& s : c->op_segs)
    if (rc == PCOA_OK && s.rows > 0) rc = pcoa_accumulate_bits(tmp, s.p, s.rows, operator_pitch_words(c->n), 1);
  if (rc == PCOA_OK) rc = pcoa_compute(tmp, num_pc, out_components, out_eigenvalues, out_nonzero_rows);
  if (rc != PCOA_OK) c->last_error = "operator compute: temporary engine: " + tmp->last_error;
  c->eig_method = tmp->eig_method;
  c->eig_dense_form = tmp->eig_dense_form;
  pcoa_destroy(tmp);
  (void)hipSetDevice(c->device);
  return rc;
}

}  // namespace

namespace pcoa {

int64_t operator_store_bytes(const pcoa_ctx* c) { return c->is_operator ? (int64_t)c->op_segs.size() * seg_bytes(c) : 0; }

// The store has room for nv more rows: every segment they need is allocated now, and a failed allocation leaves the store as
// it was.  Rows fill the segments in order, so the room is what the segments hold beyond op_variants.
int store_grow(pcoa_ctx* c, int64_t nv) {
  const size_t held = c->op_segs.size();
  const int64_t room = (int64_t)held * c->op_seg_rows - c->op_variants;
  const int64_t fresh = nv > room ? (nv - room + c->op_seg_rows - 1) / c->op_seg_rows : 0;
  for (int64_t i = 0; i < fresh; ++i) {
    void* p = nullptr;
    const hipError_t e = dev_alloc(&p, (size_t)seg_bytes(c), c->device);
    if (e != hipSuccess) {
      while (c->op_segs.size() > held) {
        dev_free(c->op_segs.back().p);
        c->op_segs.pop_back();
      }
      (void)hipGetLastError();
      return fail(c, PCOA_ERR_OUT_OF_MEMORY, "operator store: no memory for another segment of " + std::to_string(seg_bytes(c)) +
                                                 " bytes (" + hipGetErrorString(e) + "); the store keeps the " +
                                                 std::to_string(c->op_variants) + " variants it held");
    }
    c->op_segs.push_back({static_cast<uint32_t*>(p), 0});
  }
  return PCOA_OK;
}

// Appends nv rows (written on the ctx stream by the kernels `repitch` queues) to the store.  Every segment the rows need is
// allocated before the first row moves (store_grow).
int store_append(pcoa_ctx* c, int64_t nv, const std::function<hipError_t(int64_t, int64_t, uint32_t*)>& repitch) {
  if (nv <= 0) return PCOA_OK;
  const int64_t pitch = store_pitch_words(c);
  const int rc = store_grow(c, nv);
  if (rc != PCOA_OK) return rc;
  size_t si = (size_t)(c->op_variants / c->op_seg_rows);
  int64_t done = 0;
  ScopedTimer t(c, T_PACK);
  while (done < nv) {
    pcoa_ctx::OpSegment& s = c->op_segs[si];
    const int64_t cur = std::min(nv - done, c->op_seg_rows - s.rows);
    if (cur == 0) {
      ++si;
      continue;
    }
    HIP_TRY(c, repitch(done, cur, s.p + s.rows * pitch));
    s.rows += cur;
    c->op_variants += cur;
    done += cur;
  }
  c->op_centering_set = false;
  grm_ld_drop(c);   // a keep mask (pcoa_grm_ld_prune) described the store without these rows
  grm_pcr_drop(c, 1);   // and so did a PC-Relate fit
  return PCOA_OK;
}

// nv variant-major bitset rows (device) join the store
int operator_append(pcoa_ctx* c, const uint32_t* bits_dev, int64_t nv, int64_t ld_words) {
  return store_append(c, nv, [&](int64_t done, int64_t cur, uint32_t* dst) {
    return launch_operator_append(bits_dev + done * ld_words, ld_words, cur, c->n, dst, c->stream);
  });
}

// pcoa_reset: the store is empty again; the first segment stays for the next fill
int operator_reset(pcoa_ctx* c) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  while (c->op_segs.size() > 1) {
    dev_free(c->op_segs.back().p);
    c->op_segs.pop_back();
  }
  if (!c->op_segs.empty()) c->op_segs[0].rows = 0;
  c->op_variants = 0;
  c->op_centering_set = false;
  grm_ld_drop(c);
  grm_pcr_drop(c, 2);
  HIP_TRY(c, hipMemsetAsync(c->err_flag, 0, 16, c->stream));
  return PCOA_OK;
}

// pcoa_reserve: the Lanczos workspace and the first segment
int operator_reserve(pcoa_ctx* c, int32_t num_pc) {
  int rc = PCOA_OK;
  if (num_pc > 0) {
    if ((rc = ensure_workspace(c, num_pc)) != PCOA_OK) return rc;
    if (c->n >= 32) {
      const int32_t mmax = std::min<int32_t>(c->n, 512);
      if ((rc = ensure(c, &c->lanczos_ws, &c->lanczos_cap, (int64_t)lanczos_workspace_doubles(c->n, num_pc, mmax))) != PCOA_OK) return rc;
    }
  }
  if (c->op_segs.empty()) {
    void* p = nullptr;
    HIP_TRY(c, dev_alloc(&p, (size_t)seg_bytes(c), c->device));
    c->op_segs.push_back({static_cast<uint32_t*>(p), 0});
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

void operator_destroy(pcoa_ctx* c) {
  for (auto& s : c->op_segs) dev_free(s.p);
  c->op_segs.clear();
  if (c->op_ws) dev_free(c->op_ws);
  c->op_ws = nullptr;
}

// computePca (VariantsPca.scala:198-231) over the store: row sums -> means, matrix mean, non-zero rows -> the engine's Lanczos
// with the centred product.  A pair comes back only with its true residual verified; there is no dense fallback (no matrix).
int operator_compute(pcoa_ctx* c, int32_t num_pc, double* out_components, double* out_eigenvalues, int32_t* out_nonzero_rows) {
  if (c->n < 32) return operator_compute_small(c, num_pc, out_components, out_eigenvalues, out_nonzero_rows);
  const double t0 = wall_now();
  int rc = check_device_flags(c);
  if (rc != PCOA_OK) return rc;
  if ((rc = ensure_workspace(c, num_pc)) != PCOA_OK) return rc;
  if ((rc = operator_centering(c)) != PCOA_OK) return rc;
  OpWorkspace w;
  if ((rc = ensure_op_ws(c, &w)) != PCOA_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(&c->hw->nz, c->nz, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  std::string mv_error;
  LanczosMatvec mv = [&](const double* v, double* y) -> int {
    ScopedTimer t(c, T_OPERATOR);
    const hipError_t e = operator_product(c, w, v, y, 1);
    if (e == hipSuccess) return 0;
    mv_error = std::string("operator product: ") + hipGetErrorString(e);
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

}  // namespace pcoa

extern "C" {

int pcoa_operator_info(const pcoa_ctx* c, int64_t* variants_out, int64_t* store_bytes_out) {
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "ctx is NULL");
  const bool op = c->is_operator && !c->is_grm;
  if (variants_out) *variants_out = op ? c->op_variants : 0;
  if (store_bytes_out) *store_bytes_out = op ? operator_store_bytes(c) : 0;
  return op ? 1 : 0;
}

int pcoa_operator_row_sums(pcoa_ctx* c, int64_t* out_n) {
  CHECK_CTX(c);
  NOT_ON_GRM(c, "pcoa_operator_row_sums");
  if (!c->is_operator) return fail(c, PCOA_ERR_STATE, "not an operator ctx (pcoa_create_operator)");
  if (!out_n) return fail(c, PCOA_ERR_INVALID_ARG, "out_n is NULL");
  int rc = check_device_flags(c);
  if (rc != PCOA_OK) return rc;
  if ((rc = operator_centering(c)) != PCOA_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(out_n, c->stats + 2, sizeof(int64_t) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

int pcoa_operator_matvec_device(pcoa_ctx* c, const double* v_dev, double* y_dev, int centred) {
  CHECK_CTX(c);
  NOT_ON_GRM(c, "pcoa_operator_matvec_device");
  if (!c->is_operator) return fail(c, PCOA_ERR_STATE, "not an operator ctx (pcoa_create_operator)");
  if (!v_dev || !y_dev) return fail(c, PCOA_ERR_INVALID_ARG, "v_dev or y_dev is NULL");
  int rc = check_device_flags(c);
  if (rc != PCOA_OK) return rc;
  if ((rc = ensure_workspace(c, 1)) != PCOA_OK) return rc;   // (the centring vectors: also the uncentred finish takes their addresses)
  if (centred && (rc = operator_centering(c)) != PCOA_OK) return rc;
  OpWorkspace w;
  if ((rc = ensure_op_ws(c, &w)) != PCOA_OK) return rc;
  {
    ScopedTimer t(c, T_OPERATOR);
    HIP_TRY(c, operator_product(c, w, v_dev, y_dev, centred ? 1 : 0));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // y_dev is ready for the caller's own stream / collective
  return PCOA_OK;
}

}  // extern "C"
