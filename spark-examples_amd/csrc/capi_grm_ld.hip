// capi_grm_ld.hip -- pcoa_grm_ld_*: LD pruning of a GRM ctx's resident store by the r^2 of the dosages (the rule is
// stated at the block of pcoa.h, the kernels in grm_ld.hip).  The prune is a pass over the store that ends in a keep mask; the
// mask enters used_v in grm_weights_kernel, so every consumer of the weights sees the pruned store and no row moves.  A chunk
// (<= C rows) at a time:
//   the chunk's rows and the min(window, rows in front of it) rows before them are copied out of the segments into a contiguous
//   work buffer [window + C][pitch] (capi_ld.hip's arrangement; a window may span any number of segment boundaries)  ->  reach
//   (the distances at which an earlier row exists behind the last break)  ->  band  ->  ld.hip's resolve wave and scan, unchanged,
//   fed the unmasked used_v as a 0 / 1 "count" with n = 2: 0 < used < 2 is exactly "candidate".
// Every buffer of the pass is allocated before the first kernel and freed at the end; the new mask is built beside an installed
// one and replaces it only when the whole pass is through, so an error leaves the earlier mask in force.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace {

constexpr int64_t kChunkRows = (int64_t)1 << 16;     // rows per chunk at most
constexpr int64_t kChunkBytes = (int64_t)256 << 20;  // and bytes of rows per chunk

const char* kind_of(const pcoa_ctx* c) {
  if (c->is_strip) return "a strip owner (pcoa_create_strip)";
  if (c->is_operator) return "an operator ctx (pcoa_create_operator)";
  return "a full engine (pcoa_create)";
}

// PCOA_OK, or the PCOA_ERR_STATE of a ctx that has no GRM store with weights of its own
int check_kind(pcoa_ctx* c, const char* call) {
  if (!c->is_grm)
    return fail(c, PCOA_ERR_STATE, std::string(call) + ": not a GRM ctx (pcoa_create_grm) but " + kind_of(c) +
                                       ": there is no genotype store to prune");
  if (c->is_grm_study)
    return fail(c, PCOA_ERR_STATE, std::string(call) + ": a GRM study ctx (pcoa_create_grm_study) holds the genotypes of study samples and "
                                                       "no weights of its own; prune the panel's ctx, the study is placed with the panel's used variants");
  return PCOA_OK;
}

// the buffers of one pass
struct Work {
  std::vector<void*> held;
  ~Work() {
    for (void* p : held) dev_free(p);
  }
  template <typename T>
  int get(pcoa_ctx* c, T** out, int64_t count) {
    void* p = nullptr;
    const hipError_t e = dev_alloc(&p, sizeof(T) * (size_t)std::max<int64_t>(count, 1), c->device);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, PCOA_ERR_OUT_OF_MEMORY, std::string("pcoa_grm_ld_prune: no memory for the work buffers (") + hipGetErrorString(e) +
                                                 "); the ctx, the store and an earlier mask are as they were");
    }
    held.push_back(p);
    *out = static_cast<T*>(p);
    return PCOA_OK;
  }
};

// store rows [a, b) -> dst, contiguous (queued on the ctx stream)
hipError_t copy_rows(const pcoa_ctx* c, int64_t a, int64_t b, uint32_t* dst) {
  const int64_t pitch = store_pitch_words(c);
  int64_t row0 = 0;
  for (const auto& s : c->op_segs) {
    const int64_t lo = std::max(a, row0), hi = std::min(b, row0 + s.rows);
    if (lo < hi) {
      const hipError_t e = hipMemcpyAsync(dst + (lo - a) * pitch, s.p + (lo - row0) * pitch, sizeof(uint32_t) * (size_t)((hi - lo) * pitch),
                                          hipMemcpyDeviceToDevice, c->stream);
      if (e != hipSuccess) return e;
    }
    row0 += s.rows;
  }
  return hipSuccess;
}

}  // namespace

extern "C" {

int pcoa_grm_ld_prune(pcoa_ctx* c, int32_t window, double r2_max, const int64_t* breaks, int64_t n_breaks, int64_t* candidates_out,
                      int64_t* kept_out) {
  CHECK_CTX(c);
  int rc = check_kind(c, "pcoa_grm_ld_prune");
  if (rc != PCOA_OK) return rc;
  if (window < 1 || window > PCOA_LD_MAX_WINDOW)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_ld_prune: window = " + std::to_string(window) + " is outside [1, " +
                                             std::to_string(PCOA_LD_MAX_WINDOW) + "]");
  if (!(r2_max >= 0.0 && r2_max <= 1.0))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_ld_prune: r2_max = " + std::to_string(r2_max) + " is outside [0, 1]");
  if (n_breaks < 0 || (n_breaks > 0 && !breaks))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_ld_prune: breaks is NULL with n_breaks > 0, or n_breaks < 0");
  const int64_t V = c->op_variants;
  for (int64_t i = 0; i < n_breaks; ++i)
    if (breaks[i] <= 0 || breaks[i] >= V || (i > 0 && breaks[i] <= breaks[i - 1]))
      return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_ld_prune: breaks[" + std::to_string(i) + "] = " + std::to_string(breaks[i]) +
                                               ": the breaks must be strictly increasing row indices inside (0, " + std::to_string(V) + ")");
  if ((int64_t)c->n >= ((int64_t)1 << 28))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_ld_prune: N = " + std::to_string(c->n) + " samples do not fit the int32 sums of a pair (N < 2^28)");
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;

  const int64_t pitch = store_pitch_words(c), W = window, ew = (W + 31) / 32;
  const int64_t chunk = std::max<int64_t>(1, std::min(std::min(kChunkRows, kChunkBytes / (pitch * 4)), std::max<int64_t>(V, 1)));
  Work w;
  uint32_t *wb = nullptr, *ex = nullptr, *flags = nullptr, *kbits = nullptr;
  int32_t *reach = nullptr, *pos = nullptr;
  int64_t *out2 = nullptr, *brk = nullptr;
  uint8_t* keep = nullptr;
  if ((rc = w.get(c, &wb, (W + chunk) * pitch)) != PCOA_OK || (rc = w.get(c, &ex, chunk * ew)) != PCOA_OK ||
      (rc = w.get(c, &flags, 64)) != PCOA_OK || (rc = w.get(c, &kbits, chunk / 32 + 2)) != PCOA_OK ||
      (rc = w.get(c, &reach, chunk)) != PCOA_OK || (rc = w.get(c, &pos, chunk)) != PCOA_OK || (rc = w.get(c, &out2, 2)) != PCOA_OK ||
      (rc = w.get(c, &brk, n_breaks)) != PCOA_OK || (rc = w.get(c, &keep, V)) != PCOA_OK)
    return rc;
  // (an installed mask has V rows already -- an append would have dropped it -- so this never discards one)
  if ((rc = ensure(c, &c->grm_keep, &c->grm_keep_cap, V)) != PCOA_OK) return rc;

  const int32_t* used = nullptr;   // the candidates: used_v under the current min_maf, judged without an installed mask
  if ((rc = grm_unmasked_used(c, &used)) != PCOA_OK) return rc;
  if (n_breaks > 0) HIP_TRY(c, hipMemcpyAsync(brk, breaks, sizeof(int64_t) * (size_t)n_breaks, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(flags, 0, sizeof(uint32_t) * 64, c->stream));

  int64_t kept = 0, not_cand = 0;
  for (int64_t v0 = 0; v0 < V; v0 += chunk) {
    const int64_t vc = std::min(chunk, V - v0), T = std::min(W, v0);
    HIP_TRY(c, copy_rows(c, v0 - T, v0 + vc, wb + (W - T) * pitch));
    {
      ScopedTimer t(c, T_GRM_LD_BAND);
      HIP_TRY(c, launch_grm_ld_reach(brk, n_breaks, v0, vc, window, reach, c->stream));
      HIP_TRY(c, launch_grm_ld_band(wb, reach, vc, c->n, window, r2_max, ex, c->stream));
    }
    {
      ScopedTimer t(c, T_GRM_LD_RESOLVE);
      HIP_TRY(c, launch_ld_resolve(ex, used + v0, vc, 2, window, v0, flags, kbits, c->stream));
    }
    {
      ScopedTimer t(c, T_GRM_LD_SCAN);
      HIP_TRY(c, launch_ld_scan(kbits, v0, used + v0, vc, 2, keep + v0, pos, out2, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(c->hw->ld, out2, sizeof(int64_t) * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    kept += c->hw->ld[0];
    not_cand += c->hw->ld[1];
  }

  // the pass is through: the new mask replaces an installed one
  if (V > 0) HIP_TRY(c, hipMemcpyAsync(c->grm_keep, keep, (size_t)V, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->grm_keep_set = true;
  c->grm_weights_set = false;
  int64_t pairs = 0, start = 0;   // sum of reach over the rows, stretch by stretch
  for (int64_t i = 0; i <= n_breaks; ++i) {
    const int64_t end = i < n_breaks ? breaks[i] : V, len = end - start;
    pairs += len <= W ? len * (len - 1) / 2 : W * (W - 1) / 2 + (len - W) * W;
    start = end;
  }
  c->grm_ld_rows = V;
  c->grm_ld_cand = V - not_cand;
  c->grm_ld_kept = kept;
  c->grm_ld_pairs = pairs;
  if (candidates_out) *candidates_out = V - not_cand;
  if (kept_out) *kept_out = kept;
  return PCOA_OK;
}

int pcoa_grm_ld_mask(pcoa_ctx* c, int64_t first_variant, int64_t n_variants, uint8_t* out) {
  CHECK_CTX(c);
  int rc = check_kind(c, "pcoa_grm_ld_mask");
  if (rc != PCOA_OK) return rc;
  if (!c->grm_keep_set)
    return fail(c, PCOA_ERR_STATE, "pcoa_grm_ld_mask: no keep mask is installed (pcoa_grm_ld_prune has not run, or an append, pcoa_reset, "
                                   "another min_maf or pcoa_grm_ld_clear dropped its mask)");
  if (first_variant < 0 || n_variants < 0 || first_variant > c->op_variants || n_variants > c->op_variants - first_variant)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_ld_mask: rows [" + std::to_string(first_variant) + ", " +
                                             std::to_string(first_variant + n_variants) + ") are not inside the store's " +
                                             std::to_string(c->op_variants));
  if (n_variants > 0 && !out) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_grm_ld_mask: out is NULL");
  if (n_variants == 0) return PCOA_OK;
  HIP_TRY(c, hipMemcpyAsync(out, c->grm_keep + first_variant, (size_t)n_variants, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

int pcoa_grm_ld_clear(pcoa_ctx* c) {
  CHECK_CTX(c);
  const int rc = check_kind(c, "pcoa_grm_ld_clear");
  if (rc != PCOA_OK) return rc;
  grm_ld_drop(c);
  return PCOA_OK;
}

int pcoa_get_grm_ld_stats(pcoa_ctx* c, pcoa_grm_ld_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_grm_ld_stats full;
  std::memset(&full, 0, sizeof(full));
  full.grm_ld_variants = c->grm_ld_rows;
  full.grm_ld_candidates = c->grm_ld_cand;
  full.grm_ld_kept = c->grm_ld_kept;
  full.grm_ld_pairs = c->grm_ld_pairs;
  full.grm_ld_band_seconds = c->tsec[T_GRM_LD_BAND];
  full.grm_ld_resolve_seconds = c->tsec[T_GRM_LD_RESOLVE];
  full.grm_ld_scan_seconds = c->tsec[T_GRM_LD_SCAN];
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
