// capi_pairs.hip -- pcoa_similar_pairs: the screen of a stored S for duplicate and related sample pairs.
// The rule (pairs.hip restates it on the device; variants_pca.py's related_pairs_rule is the numpy statement): with
// d_i = S(i, i), S(i, j) the total entry and U = d_i + d_j - S(i, j), the pair (i, j), i < j, is reported iff U > 0 and
// (double)S(i, j) >= min_jaccard * (double)U.  Arguments are validated on the host before anything touches a device; the ctx
// is finalized and its input checks are read; every scratch buffer is allocated before the first launch and freed before
// the call returns, so a failure leaves nothing behind and the ctx usable.
#include <cmath>
#include <cstring>
#include <string>

#include "pcoa_ctx.h"

using namespace pcoa;

extern "C" {

int pcoa_similar_pairs(pcoa_ctx* c, double min_jaccard, pcoa_pair* out_pairs, int64_t capacity, int64_t* n_found_out,
                       int64_t* out_diag) {
  if (!c) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_similar_pairs: ctx is NULL");
  if (!n_found_out) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_similar_pairs: n_found_out is NULL");
  if (capacity < 0) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_similar_pairs: capacity = " + std::to_string(capacity) + " is negative");
  if (capacity > 0 && !out_pairs)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_similar_pairs: out_pairs is NULL with capacity = " + std::to_string(capacity) +
                                         " (capacity 0 is the count-only call)");
  if (!std::isfinite(min_jaccard) || !(min_jaccard > 0.0) || min_jaccard > 1.0)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_similar_pairs: min_jaccard = " + std::to_string(min_jaccard) +
                                         " is not a finite number in (0, 1]");
  NOT_ON_OPERATOR(c, "pcoa_similar_pairs");
  if (c->is_strip)
    return fail(c, PCOA_ERR_STATE, "pcoa_similar_pairs: a strip owner holds N x cols of S, not the diagonal and the upper triangle "
                                   "the screen reads; use a full engine (pcoa_create) for this call");
  if (c->n > kPairsMaxSamples) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_similar_pairs: more than 2^30 samples");
  CHECK_CTX(c);
  int rc = finalize_impl(c);
  if (rc == PCOA_OK) rc = check_device_flags(c);   // never screen an S that an input check has invalidated (synchronises)
  if (rc != PCOA_OK) return rc;

  const int32_t n = c->n;
  const size_t ntiles = (size_t)pairs_tiles(n);
  const int64_t most = (int64_t)n * (int64_t)(n - 1) / 2;   // the rule cannot report more pairs than there are
  const int64_t cap_dev = std::min(capacity, most);
  // everything the launches need, before the first of them: diag [n], rowoff [n + 1] and the write pass's entry counter in one
  // int64 block, the counts, the pairs
  int64_t* words = nullptr;
  int32_t* cnt = nullptr;
  pcoa_pair* pairs_dev = nullptr;
  auto release = [&]() {
    dev_free(words);
    dev_free(cnt);
    dev_free(pairs_dev);
    words = nullptr;
    cnt = nullptr;
    pairs_dev = nullptr;
  };
  auto alloc_bail = [&](hipError_t e, const char* what) {
    release();
    return hip_fail(c, e, what);   // hipErrorOutOfMemory comes back as PCOA_ERR_OUT_OF_MEMORY
  };
  hipError_t e;
  if ((e = dev_alloc((void**)&words, sizeof(int64_t) * (2 * (size_t)n + 2), c->device)) != hipSuccess)
    return alloc_bail(e, "the diagonal and the row offsets");
  if ((e = dev_alloc((void**)&cnt, sizeof(int32_t) * (size_t)n * ntiles, c->device)) != hipSuccess)
    return alloc_bail(e, "the (row, tile) counts");
  if (cap_dev > 0 && (e = dev_alloc((void**)&pairs_dev, sizeof(pcoa_pair) * (size_t)cap_dev, c->device)) != hipSuccess)
    return alloc_bail(e, "the pairs");
  int64_t* diag = words;
  int64_t* rowoff = words + n;                                             // n + 1 entries
  unsigned long long* entries_read = (unsigned long long*)(words + 2 * (size_t)n + 1);
  // once a launch is queued the buffers are only freed behind the stream
  auto hip_bail = [&](hipError_t err, const char* what) {
    (void)hipStreamSynchronize(c->stream);
    release();
    return hip_fail(c, err, what);
  };
  const int64_t elem_bytes = c->s64 ? (int64_t)(sizeof(int32_t) + sizeof(int64_t)) : (int64_t)sizeof(int32_t);
  {
    ScopedTimer t(c, T_PAIRS);
    if ((e = hipMemsetAsync(entries_read, 0, sizeof(unsigned long long), c->stream)) != hipSuccess) return hip_bail(e, "hipMemsetAsync");
    if ((e = launch_pairs_diag(c->s32, c->s64, n, diag, c->stream)) != hipSuccess) return hip_bail(e, "pairs_diag_kernel");
    if ((e = launch_pairs_count(c->s32, c->s64, n, diag, min_jaccard, cnt, c->stream)) != hipSuccess)
      return hip_bail(e, "pairs_count_kernel");
    if ((e = launch_pairs_scan(cnt, n, rowoff, c->stream)) != hipSuccess) return hip_bail(e, "pairs scan kernels");
    if (cap_dev > 0 &&
        (e = launch_pairs_write(c->s32, c->s64, n, diag, min_jaccard, cnt, rowoff, cap_dev, pairs_dev, entries_read, c->stream)) !=
            hipSuccess)
      return hip_bail(e, "pairs_write_kernel");
  }
  // n_found and the entry counter land in the ctx's pinned words
  if ((e = hipMemcpyAsync(&c->hw->coll[0], rowoff + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(n_found)");
  if ((e = hipMemcpyAsync(&c->hw->coll[1], entries_read, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(entries read)");
  if (out_diag && (e = hipMemcpyAsync(out_diag, diag, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(diag)");
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  const int64_t n_found = c->hw->coll[0];
  const int64_t reread = c->hw->coll[1];
  if (n_found < 0 || n_found > most) {   // cannot happen; never copy by a count that is not one
    release();
    return fail(c, PCOA_ERR_HIP, "pcoa_similar_pairs: the scan returned " + std::to_string(n_found) + " pairs of at most " + std::to_string(most));
  }
  const int64_t written = std::min(n_found, cap_dev);
  if (written > 0) {
    if ((e = hipMemcpyAsync(out_pairs, pairs_dev, sizeof(pcoa_pair) * (size_t)written, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
      return hip_bail(e, "hipMemcpyAsync(pairs)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  }
  release();
  c->pairs_bytes += elem_bytes * (pairs_count_pass_entries(n) + reread);
  c->pairs_calls += 1;
  *n_found_out = n_found;
  return PCOA_OK;
}

int pcoa_get_pairs_stats(pcoa_ctx* c, pcoa_pairs_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_pairs_stats full;
  std::memset(&full, 0, sizeof(full));
  full.pairs_seconds = c->tsec[T_PAIRS];
  full.pairs_bytes = c->pairs_bytes;
  full.pairs_calls = c->pairs_calls;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
