// capi_king.hip -- the KING-robust kinship screen from PLINK genotypes (the kernels and the rule: king.hip).
// Five ordinary full engines, the PLANES, hold the Gram matrices of the genotype-class bitsets H, M, H u M, R, A (PCOA_KING_*);
// the caller creates and owns them -- the companion pattern of capi_complete.hip, generalised.  pcoa_accumulate_plink_bed_king
// feeds the five from one read of the raw .bed rows, through the row feed (row_feed.h) of planes[0]; pcoa_king_pairs screens the
// upper triangle of the five matrices on planes[0]'s stream.  Arguments are validated on the host before anything touches a
// device and every refusal is reported on planes[0]; every scratch buffer of the screen is allocated before the first launch
// and freed before the call returns, so a failure leaves nothing behind and the planes usable.
#include <cmath>
#include <cstring>
#include <string>

#include "pcoa_ctx.h"
#include "row_feed.h"

using namespace pcoa;

namespace pcoa {

void king_destroy(pcoa_ctx* c) {
  if (c->king_read_pending)   // the other planes' pre-passes may still be reading the rows
    for (int p = 1; p < PCOA_KING_PLANES; ++p)
      if (c->king_read[p]) (void)hipEventSynchronize(c->king_read[p]);
  c->king_read_pending = false;
  if (c->king_bits) dev_free(c->king_bits);
  if (c->king_decoded) (void)hipEventDestroy(c->king_decoded);
  for (int p = 0; p < PCOA_KING_PLANES; ++p) {
    if (c->king_read[p]) (void)hipEventDestroy(c->king_read[p]);
    c->king_read[p] = nullptr;
  }
  c->king_bits = nullptr;
  c->king_bits_cap = 0;
  c->king_decoded = nullptr;
}

}  // namespace pcoa

namespace {

const char* const kPlaneName[PCOA_KING_PLANES] = {"PCOA_KING_HET", "PCOA_KING_MISSING", "PCOA_KING_HET_OR_MISSING", "PCOA_KING_HOM_A1",
                                                  "PCOA_KING_HOM_A2"};

std::string plane_name(int p) { return "planes[" + std::to_string(p) + "] (" + kPlaneName[p] + ")"; }

// what both calls ask of the five planes; no device work.  Reported on planes[0] (the thread's error where there is none)
int check_planes(pcoa_ctx* const* planes, const std::string& fn) {
  if (!planes) return fail(nullptr, PCOA_ERR_INVALID_ARG, fn + "planes is NULL");
  pcoa_ctx* c0 = planes[0];
  for (int p = 0; p < PCOA_KING_PLANES; ++p)
    if (!planes[p]) return fail(c0, PCOA_ERR_INVALID_ARG, fn + plane_name(p) + " is NULL");
  for (int p = 0; p < PCOA_KING_PLANES; ++p)
    for (int q = p + 1; q < PCOA_KING_PLANES; ++q)
      if (planes[p] == planes[q])
        return fail(c0, PCOA_ERR_INVALID_ARG, fn + plane_name(p) + " and " + plane_name(q) + " are the same ctx: five engines are needed");
  for (int p = 0; p < PCOA_KING_PLANES; ++p) {
    const pcoa_ctx* c = planes[p];
    if (c->is_grm) return fail(c0, PCOA_ERR_STATE, fn + plane_name(p) + " is a GRM ctx (pcoa_create_grm), which holds no S; use a full engine (pcoa_create)");
    if (c->is_operator || c->is_strip)
      return fail(c0, PCOA_ERR_INVALID_ARG, fn + plane_name(p) + " is " +
                                                (c->is_operator ? "an operator ctx (pcoa_create_operator)" : "a strip owner (pcoa_create_strip)") +
                                                ", which holds no full S; use a full engine (pcoa_create)");
    if (!c->use_i8)
      return fail(c0, PCOA_ERR_INVALID_ARG, fn + plane_name(p) + " is a PCOA_FLAG_GRAM_F32_MFMA engine: the planes take bitsets and "
                                                                  "need a packed-operand engine");
    if (c->n != c0->n)
      return fail(c0, PCOA_ERR_INVALID_ARG, fn + plane_name(p) + " has N = " + std::to_string(c->n) + " samples, planes[0] has " +
                                                std::to_string(c0->n));
    if (c->device != c0->device)
      return fail(c0, PCOA_ERR_INVALID_ARG, fn + plane_name(p) + " is on device " + std::to_string(c->device) + ", planes[0] on device " +
                                                std::to_string(c0->device) + ": different devices");
  }
  return PCOA_OK;
}

}  // namespace

extern "C" {

// pcoa_accumulate_plink_bed through the row feed of planes[0] with the five-plane decode: the raw rows cross the link once, one
// kernel reads them once and writes the five bitset rows into c->king_bits.  Plane 0's rows go into c on its stream, plane p's
// into planes[p] on ITS stream:
//   king_decoded   recorded on c's stream behind the decode; the streams of the planes 1 - 4 wait for it before their pre-pass
//   king_read[p]   recorded on plane p's stream behind that pre-pass; c's stream waits for the four before the next decode
//                  rewrites king_bits (in this call or a later one)
// No host wait beyond the existing call's.
int pcoa_accumulate_plink_bed_king(pcoa_ctx* const* planes, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes,
                                   int is_device_ptr) {
  const char* fn = "pcoa_accumulate_plink_bed_king: ";
  int rc = check_planes(planes, fn);
  if (rc != PCOA_OK) return rc;
  pcoa_ctx* c = planes[0];
  if (n_variants < 0 || (n_variants > 0 && !bed_rows)) return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "bed_rows is NULL or n_variants < 0");
  if ((rc = check_row_bytes(c, fn, row_bytes)) != PCOA_OK) return rc;
  if ((rc = check_bed_source(c, fn, is_device_ptr, true)) != PCOA_OK) return rc;
  CHECK_CTX(c);
  if (n_variants == 0) return PCOA_OK;
  const int64_t words = words_of(c);
  // a chunk: at most 2^17 rows, and no more than five plane buffers of 1 GiB together hold
  const int64_t by_bytes = std::max<int64_t>(1, ((int64_t)1 << 30) / (PCOA_KING_PLANES * words * 4));
  const int64_t rows_cap = std::min(std::min<int64_t>(n_variants, (int64_t)1 << 17), by_bytes);
  const int64_t plane_words = rows_cap * words;
  if (c->king_read_pending && PCOA_KING_PLANES * plane_words > c->king_bits_cap) {   // the buffer is about to be replaced: its readers first
    for (int p = 1; p < PCOA_KING_PLANES; ++p) HIP_TRY(c, hipEventSynchronize(c->king_read[p]));
    c->king_read_pending = false;
  }
  if ((rc = ensure(c, &c->king_bits, &c->king_bits_cap, PCOA_KING_PLANES * plane_words)) != PCOA_OK) return rc;
  if (!c->king_decoded) HIP_TRY(c, hipEventCreateWithFlags(&c->king_decoded, hipEventDisableTiming));
  for (int p = 1; p < PCOA_KING_PLANES; ++p)
    if (!c->king_read[p]) HIP_TRY(c, hipEventCreateWithFlags(&c->king_read[p], hipEventDisableTiming));
  KingPlaneRows out;
  for (int p = 0; p < PCOA_KING_PLANES; ++p) out.p[p] = c->king_bits + p * plane_words;
  return feed_bed(
      c, bed_rows, n_variants, row_bytes, rows_cap, is_device_ptr, true,
      [&](const uint8_t* src, int64_t, int64_t rows) -> int {
        if (c->king_read_pending)
          for (int p = 1; p < PCOA_KING_PLANES; ++p) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->king_read[p], 0));
        {
          ScopedTimer t(c, T_DENSIFY);
          HIP_TRY(c, launch_plink_bed_to_king_planes(src, row_bytes, rows, c->n, words, out, c->stream));
        }
        HIP_TRY(c, hipEventRecord(c->king_decoded, c->stream));
        return PCOA_OK;
      },
      [&](int64_t, int64_t rows) -> int {
        int rc2 = gram_device_bits(c, out.p[0], rows, words, false);
        if (rc2 != PCOA_OK) return fail(c, rc2, std::string(fn) + plane_name(0) + ": " + c->last_error);
        for (int p = 1; p < PCOA_KING_PLANES; ++p) {
          pcoa_ctx* q = planes[p];
          HIP_TRY(c, hipStreamWaitEvent(q->stream, c->king_decoded, 0));
          c->king_read_pending = true;   // (from here on plane p's stream holds work that reads the buffer)
          if ((rc2 = gram_device_bits(q, out.p[p], rows, words, false)) != PCOA_OK)
            return fail(c, rc2, std::string(fn) + plane_name(p) + ": " + q->last_error);
          HIP_TRY(c, hipEventRecord(c->king_read[p], q->stream));
        }
        return PCOA_OK;
      });
}

int pcoa_king_pairs(pcoa_ctx* const* planes, double min_kinship, pcoa_king_pair* out_pairs, int64_t capacity, int64_t* n_found_out,
                    int64_t* n_variants_out, int64_t* out_het) {
  const char* fn = "pcoa_king_pairs: ";
  int rc = check_planes(planes, fn);
  if (rc != PCOA_OK) return rc;
  pcoa_ctx* c = planes[0];
  if (!n_found_out) return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "n_found_out is NULL");
  if (capacity < 0) return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "capacity = " + std::to_string(capacity) + " is negative");
  if (capacity > 0 && !out_pairs)
    return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "out_pairs is NULL with capacity = " + std::to_string(capacity) +
                                         " (capacity 0 is the count-only call)");
  if (!std::isfinite(min_kinship) || !(min_kinship > 0.0) || min_kinship > 0.5)
    return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "min_kinship = " + std::to_string(min_kinship) +
                                         " is not a finite number in (0, 0.5]");
  if (c->n > kPairsMaxSamples) return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "more than 2^30 samples");
  CHECK_CTX(c);
  // never screen an S that an input check has invalidated (this synchronises each plane's stream: everything a plane was fed is
  // in its S before a kernel of c's stream reads it)
  KingMatrices g;
  for (int p = 0; p < PCOA_KING_PLANES; ++p) {
    pcoa_ctx* q = planes[p];
    rc = finalize_impl(q);
    if (rc == PCOA_OK) rc = check_device_flags(q);
    if (rc != PCOA_OK) return fail(c, rc, std::string(fn) + plane_name(p) + ": " + q->last_error);
    if (q->s64)
      return fail(c, PCOA_ERR_STATE, std::string(fn) + plane_name(p) + " has an int64 part (more than 2^30 variants accumulated into "
                                     "it): the kinship screen over an int64 plane is not built");
    g.p[p] = q->s32;
  }

  const int32_t n = c->n;
  const size_t ntiles = (size_t)pairs_tiles(n);
  const int64_t most = (int64_t)n * (int64_t)(n - 1) / 2;   // the rule cannot report more pairs than there are
  const int64_t cap_dev = std::min(capacity, most);
  // everything the launches need, before the first of them: h [n], hm [n], rowoff [n + 1], the write pass's entry counter, V
  // and the four flag words in one int64 block, the counts, the pairs
  int64_t* words = nullptr;
  int32_t* cnt = nullptr;
  pcoa_king_pair* pairs_dev = nullptr;
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
  static_assert(kKingFlagWords * sizeof(int32_t) == 2 * sizeof(int64_t), "the flag words take two int64 of the block");
  hipError_t e;
  if ((e = dev_alloc((void**)&words, sizeof(int64_t) * (3 * (size_t)n + 5), c->device)) != hipSuccess)
    return alloc_bail(e, "the diagonals and the row offsets");
  if ((e = dev_alloc((void**)&cnt, sizeof(int32_t) * (size_t)n * ntiles, c->device)) != hipSuccess)
    return alloc_bail(e, "the (row, tile) counts");
  if (cap_dev > 0 && (e = dev_alloc((void**)&pairs_dev, sizeof(pcoa_king_pair) * (size_t)cap_dev, c->device)) != hipSuccess)
    return alloc_bail(e, "the pairs");
  int64_t* h = words;
  int64_t* hm = words + n;
  int64_t* rowoff = words + 2 * (size_t)n;                                 // n + 1 entries
  int64_t* tail = words + 3 * (size_t)n + 1;                               // {entries read, V, flags, flags}
  unsigned long long* entries_read = (unsigned long long*)tail;
  int64_t* v_dev = tail + 1;
  int32_t* flag = reinterpret_cast<int32_t*>(tail + 2);
  // once a launch is queued the buffers are only freed behind the stream
  auto hip_bail = [&](hipError_t err, const char* what) {
    (void)hipStreamSynchronize(c->stream);
    release();
    return hip_fail(c, err, what);
  };
  {
    ScopedTimer t(c, T_KING);
    if ((e = hipMemsetAsync(tail, 0, 4 * sizeof(int64_t), c->stream)) != hipSuccess) return hip_bail(e, "hipMemsetAsync");
    if ((e = launch_king_diag(g, n, h, hm, v_dev, flag, c->stream)) != hipSuccess) return hip_bail(e, "king_diag_kernel");
    if ((e = launch_king_count(g, n, h, hm, v_dev, min_kinship, cnt, flag, c->stream)) != hipSuccess) return hip_bail(e, "king_count_kernel");
    if ((e = launch_pairs_scan(cnt, n, rowoff, c->stream)) != hipSuccess) return hip_bail(e, "pairs scan kernels");
    if (cap_dev > 0 && (e = launch_king_write(g, n, h, hm, v_dev, min_kinship, cnt, rowoff, cap_dev, pairs_dev, entries_read,
                                              c->stream)) != hipSuccess)
      return hip_bail(e, "king_write_kernel");
  }
  // the flags, V, n_found and the entry counter land in the ctx's pinned words
  if ((e = hipMemcpyAsync(c->hw->kflag, flag, sizeof(int32_t) * kKingFlagWords, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(flags)");
  if ((e = hipMemcpyAsync(&c->hw->king[0], v_dev, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(V)");
  if ((e = hipMemcpyAsync(&c->hw->king[1], rowoff + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(n_found)");
  if ((e = hipMemcpyAsync(&c->hw->king[2], entries_read, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(entries read)");
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  const int64_t v = c->hw->king[0], n_found = c->hw->king[1], reread = c->hw->king[2];
  const char* inconsistent = nullptr;
  if (c->hw->kflag[kKingFlagV]) inconsistent = "V = r_i + a_i + hm_i is not the same for every sample";
  else if (c->hw->kflag[kKingFlagIbs0]) inconsistent = "ibs0 < 0 for some pair";
  else if (c->hw->kflag[kKingFlagHetSum]) inconsistent = "het_sum < 0 for some pair";
  else if (c->hw->kflag[kKingFlagSHm]) inconsistent = "s_hm < 0 for some pair";
  if (inconsistent) {
    release();
    return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "the planes were not fed the same rows: " + inconsistent);
  }
  if (n_found < 0 || n_found > most) {   // cannot happen; never copy by a count that is not one
    release();
    return fail(c, PCOA_ERR_HIP, std::string(fn) + "the scan returned " + std::to_string(n_found) + " pairs of at most " + std::to_string(most));
  }
  const int64_t written = std::min(n_found, cap_dev);
  if (written > 0 &&
      (e = hipMemcpyAsync(out_pairs, pairs_dev, sizeof(pcoa_king_pair) * (size_t)written, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(pairs)");
  if (out_het && (e = hipMemcpyAsync(out_het, h, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(het)");
  if ((written > 0 || out_het) && (e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  release();
  c->king_bytes += (int64_t)(PCOA_KING_PLANES * sizeof(int32_t)) * (pairs_count_pass_entries(n) + reread);
  c->king_calls += 1;
  *n_found_out = n_found;
  if (n_variants_out) *n_variants_out = v;
  return PCOA_OK;
}

int pcoa_get_king_stats(pcoa_ctx* c, pcoa_king_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_king_stats full;
  std::memset(&full, 0, sizeof(full));
  full.king_seconds = c->tsec[T_KING];
  full.king_bytes = c->king_bytes;
  full.king_calls = c->king_calls;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
